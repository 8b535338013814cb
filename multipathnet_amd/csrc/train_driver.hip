// train_driver.hip — training a VGG Fast R-CNN handle on the device (include/mpn.h mpn_frcnn_train_*): the ROI
// head with the trunk frozen, or with the trunk's last conv layers (MPN_TRAIN_CONV(k), MPN_TRAIN_TRUNK(k)); and the towers of a
// MultiPathNet handle with the trunk frozen (mpn_mpnet_train_*; section 13.9) or with the conv block above the last pooling layer
// trained through the skip pooling (mpn_mpnet_train_begin_conv; section 13.15) — two trainers over one core, one layer table
// (section 13.12) and one conv block.  Host code only: the kernels are train.hip's (train.h) and the detect path's (dense.h); the handle and what is
// shared with pipeline.hip: pipeline.h.  The state-free debug pass-throughs to the kernels: train_debug.hip.
#include <cmath>
#include <algorithm>
#include <memory>
#include <vector>

#include "pipeline.h"
#include "sampler.h"
#include "train.h"

// What *_train_add_sampled draws an image's rows into (sampler.h): the attach_proposals record of the image
// ([m] rows, regrown for the largest image seen), the sampler's two row lists, and the sampled rows the add then reads — sized at
// train_begin for max_rois rows and regrown for a larger batch_size (the overflow is refused only once the counts are known).  The
// mirrored image of a flipped add lives here too.  All slots of the training state's DeviceOwner.
struct SampleBufs {
  float *boxes = nullptr, *overlap = nullptr;      // the record
  int *corr = nullptr, *label = nullptr, *lists = nullptr;
  size_t boxes_b = 0, overlap_b = 0, corr_b = 0, label_b = 0, lists_b = 0;
  float *rois = nullptr, *gt = nullptr;            // the sampled rows
  int *labels = nullptr, *counts = nullptr;
  size_t rois_b = 0, gt_b = 0, labels_b = 0, counts_b = 0;
  float *flipped = nullptr;                        // the mirrored image [3, H, W]
  size_t flipped_b = 0;
};
// train_begin's part: the sampled-row buffers for max_rois rows and the two counts.  Plain allocations — the allocation generation is
// not bumped, so a launch graph captured before training is still replayed after it.
static bool alloc_sample_rows(SampleBufs &b, DeviceOwner &own, size_t rows) {
  b.rois_b = b.gt_b = rows * 4 * sizeof(float); b.labels_b = rows * sizeof(int); b.counts_b = 2 * sizeof(int);
  return own.alloc_slot(&b.rois, b.rois_b) == MPN_OK && own.alloc_slot(&b.gt, b.gt_b) == MPN_OK &&
         own.alloc_slot(&b.labels, b.labels_b) == MPN_OK && own.alloc_slot(&b.counts, b.counts_b) == MPN_OK;
}

// What both trainers keep between *_train_begin and *_train_end: the optimiser's settings, the pending minibatch, the dropout stream
struct TrainCore {
  float momentum = 0.f, weight_decay = 0.f, bbox_weight = 1.f;
  int head_k = 0;                      // the integral classifier the next step's loss reads (*_train_set_head); not optimiser state
  float *rois = nullptr, *gt = nullptr, *loss = nullptr;   // the pending minibatch's boxes [max_rois,4] x 2; the two loss terms
  int *labels = nullptr;
  int pending = 0, last_rows = 0;      // rows added since the last step; rows of the last step (debug tensors "train_pooled", "train_y6", "tower_train_cat", ...)
  // nn.Dropout(rate) behind every fc6 + ReLU and fc7 + ReLU (*_train_set_dropout; 0: none, no kernel).  The mask is a function of
  // (seed, step, layer, row, column) — train.h dropout_c8 —, so the stream's whole state is `seed` and `step`
  float drop_rate = 0.f, drop_scale = 1.f;   // scale = 1.0f / (1.0f - rate)
  uint32_t drop_threshold = 0;         // floor(rate * 2^32): an element is kept iff its word >= this
  long seed = 0, step = 0;             // step: the train_steps that reached the forward pass (mpn_frcnn_train_get_state / _set_state)
  SampleBufs smp;                      // *_train_add_sampled's record and sampled rows
  DeviceOwner own;                     // of every buffer of the state: *_train_end gives them back at once, not at handle destruction
};

// A Linear layer of a step.  w, b: the handle's packed weights (creation alone allocates them: no entry point replaces them while a state
// exists).  x: the layer's input, g: the gradient at its output, C8 matrices at row pitch nseg * Mp; v, vb: momentum, in the layout of the
// weight it goes with (trained layers only).  The x are the minibatch's own activations — not detect's buffers, so a detect between
// two training calls disturbs nothing.
struct LinT {
  float *w, *b; int K, N, inner, relu; float *x, *g, *v, *vb;
  float *y = nullptr, *y_rm = nullptr; // the output: a C8 matrix (the x of the layer above) or row-major (a head)
  int drop = -1;                       // >= 0: y goes through the dropout under this layer word
  float *dx = nullptr;                 // where lin_dgrad puts the gradient at x (null: not its business)
  int masked = 1;                      // x is a ReLU output behind the dropout: dx is masked with [x > 0] and scaled by 1 / (1 - rate)
  int nseg = 1;                        // > 1 (MultiPathNet's mix, PP): the valid rows are nseg segments of B at pitch Mp — the forward runs over all
};                                     // nseg * Mp rows, the update is sgd_wgrad_seg_c8 / sgd_bias_seg_c8

// The conv block of a training state — the trunk's trained conv layers conv[first] .. conv[first + kconv - 1], their saved maps and
// what their backward pass works in.  Both kinds' states hold one: the plain handle's at depth >=
// MPN_TRAIN_CONV(1), the tower handle's under mpn_mpnet_train_begin_conv(k > 0).  The layers lie above the last pooling layer, or
// (plain handle, MPN_TRAIN_TRUNK(k), k > K) with pooling layers among them: then every map has its own size (train_map)
struct ConvBlock {
  struct ConvT {
    float *v = nullptr, *vb = nullptr;       // momentum: `wpk` layout, [CoutP]
    float *dw = nullptr, *db = nullptr;      // the step's gradients, summed over the images in train_add order
    float *wpk_t = nullptr, *wino_t = nullptr, *zero_b = nullptr;  // the input gradient's convolution (pack_conv_weights_dgrad); wino_t where Cout >= 16
  };
  int kconv = 0, first = 0;
  bool dgrad_wino = true;              // the input gradients run on the forward's Winograd kernel where Cout >= 16.  The tower handle's block
                                       // takes the direct kernels instead (the Winograd form's rounding reached the
                                       // weight gradient of the layer below at 2.5 x the fp32 yardstick); the plain handle keeps its bits
  std::vector<ConvT> cl;               // [kconv], cl[j] goes with conv[first + j]
  float *acts = nullptr;               // per image: the block's input map and the kconv trained layers' outputs (before the pool where pooled), whole C8P planes,
                                       // then the pooled map of every pooled trained layer but the last (the next trained layer's input)
  size_t act_off[MPN_TRAIN_MAX_TRUNK + 1] = {}, pool_off[MPN_TRAIN_MAX_TRUNK + 1] = {}, act_img = 0; // floats: map j / pooled map j inside an image's slot; between two images' slots
  float *gmap[2] = {nullptr, nullptr}; // the gradient maps of the image being worked on (ping-pong through the layers)
  size_t gmap_bytes = 0;
  float *wtmp = nullptr, *part = nullptr;  // a layer's weights in Torch layout (x 2: W, W'); conv3x3_wgrad's partial sums
  int n_img = 0, last_img = 0;         // images pending; images of the last step (debug tensors "train_act.<i>.<j>", "tower_train_act.<i>.<j>")
  int img_h[MPN_TRAIN_MAX_IMAGES] = {}, img_w[MPN_TRAIN_MAX_IMAGES] = {}, img_row0[MPN_TRAIN_MAX_IMAGES] = {}, img_rows[MPN_TRAIN_MAX_IMAGES] = {};  // final map size, row range
  int img_nh[MPN_TRAIN_MAX_IMAGES] = {}, img_nw[MPN_TRAIN_MAX_IMAGES] = {};  // network-input size (every layer's map size follows from it)
};
using ConvT = ConvBlock::ConvT;

// The training state of a plain handle: exists between train_begin and train_end
struct TrainState : TrainCore, ConvBlock {
  LinT fc[3] = {};                     // fc6 (x: the ROI-pooled rows of the pending images), fc7, the fused cls + bbox head
  int n_fc = 1;                        // how many of them, counted from the head down, are trained
  float *head = nullptr;               // the head's output, row-major [B, (K+4)C]
  float *vtmp = nullptr;               // mpn_frcnn_train_set_state: cls and bbox momentum joined as creation joins the weights, [(K+4)C, F] + [(K+4)C]
  // ---- depth >= MPN_TRAIN_CONV(1): the conv block (ConvBlock) and what the ROI pooling's backward reads
  float *dx6 = nullptr;                // gradient at the pooled features, fc[0].x's layout
  int32_t *argmax = nullptr;           // [max_rois, C, PH, PW] of the pending rows
  float *prois = nullptr;              // [max_rois, 5] the pending rows' projected ROIs (the bins' windows)
};

// The training state of a MultiPathNet handle's towers (mpn_mpnet_train_*): exists between mpn_mpnet_train_begin
// and mpn_mpnet_train_end.  Every activation and gradient of a step lives here, none in detect's buffers.
struct TowerTrainState : TrainCore, ConvBlock {
  // The layers in forward order: per tower t its mix, fc6, fc7 (rows 3 t ..), then the K classifiers and the box regressor.
  //   mix: x the operand [Kcat64/8][PP * Mp][8], rows (bin, roi), the normalised ROI pools side by side; K = Kcat, the tower's concat width
  //        (conv5 [+ conv4] [+ conv3]); y [c5P/8][PP * Mp][8] == fc6's operand [.. >= K6_64/8][Mp][8]; no ReLU between the two
  //        (multipathnet.lua: View, Linear), so fc6's dx — the mix's g, in y's layout — is unmasked
  //   fc6: y as fc7 read it, behind the dropout under the layer word 2 t;  fc7: y the tower's columns of `cat`, word 2 t + 1, g those of `dcat`
  std::vector<LinT> lin;
  std::vector<int> bwd;                          // the rows in the backward pass's order: the heads, then per tower fc7, fc6, mix
  float *cat = nullptr, *dcat = nullptr;         // the towers' fc7 outputs side by side [T * F/8][Mp][8] (behind the dropout); the gradient there
  float *seg_part = nullptr;                     // sgd_wgrad_seg_c8's partial sums (the widest tower's)
  // ---- mpn_mpnet_train_begin_conv(k > 0): the conv block (ConvBlock) and what lies between it and the mix layers
  std::vector<float *> gx;                       // [T] the gradient at tower t's conv5 slab [c5P/8][PP * Mp][8] (the operand's rows), before nn.Normalize's backward ...
  std::vector<float *> dx5;                      // ... and behind it (conv345_unnormalized: the same buffer, the factor is 1)
  std::vector<int> regions;                      // the distinct Foveal regions of the towers, ascending
  std::vector<float *> xraw;                     // [regions] conv5's raw ROI max-pools over the region, the operand's layout (nn.Normalize's input)
  std::vector<int32_t *> argmax;                 // [regions] [max_rois, c5, PH, PW] of the pending rows
  float *pfov = nullptr;                         // [max_rois, 20] the pending rows' Foveal table (the bins' windows)
  float *g5 = nullptr;                           // per image: the gradient map at conv5's output behind the ReLU mask (debug tensor "tower_train_g5.<i>"), g5_img floats apart
  size_t g5_img = 0;
  int region_slot(int region) const { return (int)(std::find(regions.begin(), regions.end(), region) - regions.begin()); }
  LinT &mix(int t) { return lin[3 * t]; }
  LinT &fc6(int t) { return lin[3 * t + 1]; }
  LinT &cls() { return lin[lin.size() - 2]; }    // y_rm [B, K*C], g: train_loss_split's two gradient matrices
  LinT &bbox() { return lin[lin.size() - 1]; }   // y_rm [B, 4C]
};

void mpn::free_train_state(mpn_frcnn *p) {
  delete p->train;  // (its DeviceOwner gives the buffers back)
  p->train = nullptr;
  delete p->tower_train;
  p->tower_train = nullptr;
}

// MPN_CHECK_ARG / MPN_CHECK_HIP in a body that two entry points share: reported under the entry point's name `fn`
#define CHECK_ARG_AS(fn, cond) do { if (!(cond)) { set_error("%s: invalid argument: %s", fn, #cond); return MPN_EINVAL; } } while (0)
#define CHECK_HIP_AS(fn, expr) \
  do { hipError_t _e = (expr); if (_e != hipSuccess) { set_error("%s: %s failed: %s", fn, #expr, hipGetErrorString(_e)); return MPN_EHIP; } } while (0)

// The two kinds of trainer, told apart by `mpnet` in everything they share: mpn_frcnn_train_* on a plain handle's TrainState,
// mpn_mpnet_train_* on a MultiPathNet handle's TowerTrainState
static const char *kind_prefix(bool mpnet) { return mpnet ? "mpn_mpnet" : "mpn_frcnn"; }

// The handle kinds and states that cannot train, each named (as refuse_multi_pass does for the throughput forms).  Each kind refuses
// the other's handles; the order of the refusals is each kind's own.
static int refuse_train(const mpn_frcnn *p, bool mpnet, const char *fn) {
  if (mpnet && p->n_scales > 1) {  // (only a plain handle can hold one)
    set_error("%s: not supported with an image pyramid (mpn_frcnn_set_scales, %d scales), which only a plain Fast R-CNN handle holds: this entry point trains mpn_mpnet_create handles", fn, p->n_scales);
    return MPN_ESTATE;
  }
  if (mpnet && !p->is_mpnet) {
    set_error("%s: not an mpn_mpnet_create handle: a %s handle has no towers to train%s", fn, handle_kind_name(p), p->rn ? "" : " (mpn_frcnn_train_begin trains its head)");
    return MPN_ESTATE;
  }
  if (!mpnet && (p->is_mpnet || p->rn)) {
    set_error("%s: a %s handle cannot be trained: only mpn_frcnn_create's VGG Fast R-CNN head (fc6, fc7, cls + bbox) has a backward pass%s", fn, handle_kind_name(p),
              p->is_mpnet ? " here (its towers train through mpn_mpnet_train_begin)" : "");
    return MPN_ESTATE;
  }
  if (p->cfg.fc_arith != MPN_FC_FP32) {
    set_error("%s: an MPN_FC_SPLIT3 handle cannot be trained (its bf16 weight planes would go stale): create it with MPN_FC_FP32", fn);
    return MPN_ESTATE;
  }
  if (p->n_scales > 1) {
    set_error("%s: not supported with an image pyramid (mpn_frcnn_set_scales, %d scales): restore a single scale first", fn, p->n_scales);
    return MPN_ESTATE;
  }
  if (p->augment) {
    set_error("%s: not supported with horizontal-flip augmentation (mpn_frcnn_set_augment): switch it off; flip training images with mpn_image_hflip / mpn_flip_boxes", fn);
    return MPN_ESTATE;
  }
  if (p->tail_pending[0] || p->tail_pending[1]) {
    set_error("%s: a pipelined call's tail is still pending on this handle: call mpn_frcnn_flush first", fn);
    return MPN_ESTATE;
  }
  return MPN_OK;
}

// the core of the kind's state (null outside begin .. end); need_core: or a refusal
static TrainCore *core_of(mpn_frcnn *p, bool mpnet) { return mpnet ? static_cast<TrainCore *>(p->tower_train) : p->train; }
static int need_core(mpn_frcnn *p, bool mpnet, const char *fn, TrainCore **c) {
  *c = core_of(p, mpnet);
  if (*c) return MPN_OK;
  set_error("%s: no %s_train_begin on this handle", fn, kind_prefix(mpnet));
  return MPN_ESTATE;
}

// *_train_begin up to its own arguments: the handle can train and has not begun
static int begin_refusals(mpn_frcnn *p, bool mpnet, const char *fn) {
  if (int rc = refuse_train(p, mpnet, fn)) return rc;
  if (!core_of(p, mpnet)) return MPN_OK;
  set_error("%s: training has already begun on this handle (%s_train_end first)", fn, kind_prefix(mpnet));
  return MPN_ESTATE;
}
// ... and from its optimiser arguments on: checked, the device idle, taken into the new state
static int begin_core(TrainCore &c, const char *fn, float momentum, float weight_decay, float bbox_weight) {
  CHECK_ARG_AS(fn, std::isfinite(momentum) && momentum >= 0.0f && std::isfinite(weight_decay) && weight_decay >= 0.0f && std::isfinite(bbox_weight));
  CHECK_HIP_AS(fn, hipDeviceSynchronize());
  c.momentum = momentum; c.weight_decay = weight_decay; c.bbox_weight = bbox_weight;
  return MPN_OK;
}

// The core's buffers: the pending rows and, for *_train_add_sampled, the sampled rows.  Plain allocations — the allocation generation is
// not bumped, so a launch graph captured before training is still replayed after it.
static bool alloc_core(const mpn_frcnn *p, TrainCore &c) {
  const size_t M = (size_t)p->cfg.max_rois;
  return c.own.alloc(&c.rois, M * 4 * sizeof(float), true) == MPN_OK && c.own.alloc(&c.gt, M * 4 * sizeof(float), true) == MPN_OK &&
         c.own.alloc(&c.loss, 16, true) == MPN_OK && c.own.alloc(&c.labels, M * sizeof(int), true) == MPN_OK && alloc_sample_rows(c.smp, c.own, M);
}
// a trained layer's momentum
static bool alloc_momentum(DeviceOwner &own, LinT &L) {
  return own.alloc(&L.v, lin_wpk_elems(round_up(L.K, 64), L.N) * sizeof(float), true) == MPN_OK && own.alloc(&L.vb, (size_t)lin_np(L.N) * sizeof(float), true) == MPN_OK;
}

static int train_end(mpn_frcnn *p, bool mpnet, const char *fn) {
  TrainCore *c;
  if (int rc = need_core(p, mpnet, fn, &c)) return rc;
  CHECK_HIP_AS(fn, hipDeviceSynchronize());
  free_train_state(p);
  return MPN_OK;
}

static int train_set_head(mpn_frcnn *p, bool mpnet, const char *fn, int k) {
  TrainCore *c;
  if (int rc = need_core(p, mpnet, fn, &c)) return rc;
  if (k < 0 || k >= p->n_integral) {
    set_error("%s: invalid argument: head %d is outside [0, K) of this handle's K = %d integral classifiers", fn, k, p->n_integral);
    return MPN_EINVAL;
  }
  c->head_k = k;  // read by the next *_train_step
  return MPN_OK;
}

static int train_set_dropout(mpn_frcnn *p, bool mpnet, const char *fn, float rate, long seed) {
  TrainCore *c;
  if (int rc = need_core(p, mpnet, fn, &c)) return rc;
  if (!(std::isfinite(rate) && rate >= 0.0f && rate < 1.0f)) {
    set_error("%s: rate %g is outside [0, 1)", fn, (double)rate);
    return MPN_EINVAL;
  }
  c->drop_rate = rate;
  c->drop_threshold = (uint32_t)std::floor((double)rate * 4294967296.0);
  c->drop_scale = 1.0f / (1.0f - rate);
  c->seed = seed;
  return MPN_OK;
}

static LossCfg loss_cfg(const mpn_frcnn *p, const TrainCore &c) {
  LossCfg lc{};
  for (int i = 0; i < 4; ++i) { lc.mean[i] = p->cfg.bbox_mean[i]; lc.std[i] = p->cfg.bbox_std[i]; }
  lc.norm = p->cfg.bbox_std[0] != 0.0f ? 1 : 0;
  lc.bbox_weight = c.bbox_weight;
  return lc;
}

static DropoutCfg dropout_cfg(const TrainCore &c, int layer, long step) {
  return DropoutCfg{c.drop_threshold, (uint32_t)((uint64_t)c.seed & 0xffffffffu), (uint32_t)((uint64_t)c.seed >> 32), (uint32_t)layer,
                    (uint32_t)((uint64_t)step & 0xffffffffu), c.drop_scale};
}

// ---- the three passes of a step over the layer table: the launches of both kinds' Linear layers
// Forward, rows[0 .. n) in order: detect's GEMMs on the pending rows and, at a rate > 0, the dropout of the outputs that have one (the
// model is in training mode at every depth: frozen layers drop too).  A segmented layer runs over all nseg * Mp rows of its operand
// (a row's result depends on that row alone) in the one-segment canonical order.
static int lin_forward(const LinT *rows, int n, const TrainCore &c, int B, int Mp, long step, hipStream_t s) {
  int rc = MPN_OK;
  for (int i = 0; i < n && rc == MPN_OK; ++i) {
    const LinT &L = rows[i];
    rc = linear_c8(L.x, L.nseg > 1 ? L.nseg * Mp : B, L.K, L.w, L.b, L.N, L.relu, L.y, L.y_rm, s, L.nseg * Mp, nullptr, L.nseg > 1 ? 2 : 1);
    if (rc == MPN_OK && L.drop >= 0 && c.drop_rate > 0.0f) rc = dropout_c8(L.y, Mp, B, L.N, dropout_cfg(c, L.drop, step), s);
  }
  return rc;
}
// The input gradients of the rows that hand one down (dx), in `order`: all of them run before any update of the weights they read.  A
// masked row's x is what the dropout left: a dropped element is +0.0, so the kernel's [x > 0] is keep mask x ReLU mask and the
// dropout's backward is the factor 1 / (1 - rate) alone
static int lin_dgrad(const LinT *rows, const int *order, int n, const TrainCore &c, int B, int Mp, hipStream_t s) {
  const float gscale = c.drop_rate > 0.0f ? c.drop_scale : 1.0f;
  int rc = MPN_OK;
  for (int i = 0; i < n && rc == MPN_OK; ++i) {
    const LinT &L = rows[order[i]];
    if (L.dx) rc = linear_dgrad_c8(L.g, Mp, B, L.N, L.w, L.K, L.masked ? L.x : nullptr, L.dx, Mp, s, L.masked ? gscale : 1.0f);
  }
  return rc;
}
// The weight and bias updates of the trained rows (v), in `order`, in place on the packed weights detect reads.  part: the segmented form's partial sums
static int lin_update(const LinT *rows, const int *order, int n, const TrainCore &c, int B, int Mp, float lr, float *part, hipStream_t s) {
  int rc = MPN_OK;
  for (int i = 0; i < n && rc == MPN_OK; ++i) {
    const LinT &L = rows[order[i]];
    if (!L.v) continue;
    if (L.nseg > 1) {
      rc = sgd_wgrad_seg_c8(L.g, L.x, Mp, L.nseg, B, L.N, L.K, part, L.w, L.v, lr, c.momentum, c.weight_decay, s);
      if (rc == MPN_OK) rc = sgd_bias_seg_c8(L.g, Mp, L.nseg, B, L.N, L.b, L.vb, lr, c.momentum, s);
    } else {
      rc = sgd_wgrad_c8(L.g, Mp, L.x, Mp, B, L.N, L.K, L.inner, L.w, L.v, lr, c.momentum, c.weight_decay, s);
      if (rc == MPN_OK) rc = sgd_bias_c8(L.g, Mp, B, L.N, L.b, L.vb, lr, c.momentum, s);
    }
  }
  return rc;
}

// The forms of a conv layer that are derived from its master `wpk`: (forward) the Winograd and K = 36 packs detect's kernels read, rebuilt
// IN PLACE by the packers creation used from the layer unpacked to Torch layout — bit-identical to what creation would build from the
// exported weights; and, where the layer hands a gradient down (T.wpk_t), the input gradient's packs.  d_wtmp: 2 x Cout * Cin * 9 floats.
static int refresh_conv_forms(const ConvLayer &L, const ConvT &T, float *d_wtmp, bool forward, hipStream_t s) {
  int rc = unpack_conv_weights(L.wpk, nullptr, L.Cin, L.Cout, d_wtmp, nullptr, s);
  if (rc == MPN_OK && forward && L.wino) rc = pack_conv_weights_wino(d_wtmp, L.Cin, L.Cout, L.wino, s);
  if (rc == MPN_OK && forward && L.w36) rc = pack_conv_weights_first(d_wtmp, L.Cin, L.Cout, L.w36, s);
  if (rc == MPN_OK && T.wpk_t) rc = pack_conv_weights_dgrad(d_wtmp, L.Cin, L.Cout, d_wtmp + (size_t)L.Cout * L.Cin * 9, T.wpk_t, T.zero_b, T.wino_t, s);
  return rc;
}

// the size of conv[l]'s input and output maps for an H x W network input: halved (rounding up) at every pooling layer below it
static void layer_map_size(const mpn_frcnn *p, int l, int H, int W, int *h, int *w) {
  for (int i = 0; i < l; ++i) if (p->conv[i].pool) { H = (H + 1) / 2; W = (W + 1) / 2; }
  *h = H; *w = W;
}
// Saved map j of the trained block for an H x W network input, at `base` (an image's slot): j = 0 the input of conv[first], j = 1..k the
// post-ReLU output of conv[first + j - 1] before its pool; pooled: the pooled output of that layer (1 <= j < k, the layer pooled)
static Act train_map(const mpn_frcnn *p, const ConvBlock *t, float *base, int j, bool pooled, int H, int W) {
  const int l = j == 0 ? t->first : t->first + j - 1;
  int h, w;
  layer_map_size(p, pooled ? l + 1 : l, H, W, &h, &w);
  return make_act(base ? base + (pooled ? t->pool_off[j] : t->act_off[j]) : nullptr, j == 0 ? p->conv[l].Cin : p->conv[l].Cout, h, w);  // (no base: the geometry alone)
}
// the input map of trained layer j (1..k): saved map j - 1, or its pooled form where the layer below is pooled
static Act train_in_map(const mpn_frcnn *p, const ConvBlock *t, float *base, int j, int H, int W) {
  return train_map(p, t, base, j - 1, j > 1 && p->conv[t->first + j - 2].pool, H, W);
}

// K: the conv layers behind the trunk's last pooling layer (none when the trunk has no pooling layer: the block's input would be the
// image), capped at MPN_TRAIN_MAX_CONV
static int conv_layers_above_last_pool(const mpn_frcnn *p) {
  const int n_conv = (int)p->conv.size();
  int Kmax = 0;
  while (Kmax < n_conv && !p->conv[n_conv - 1 - Kmax].pool) ++Kmax;
  if (Kmax == n_conv) Kmax = 0;
  return std::min(Kmax, (int)MPN_TRAIN_MAX_CONV);
}
// MPN_TRAIN_* -> the trained layers: the last n_fc Linear layers and, below fc6, the conv layers conv[first] .. conv[first + kconv - 1]
// (kconv == 0: none) — or a refusal
static int parse_train_depth(const mpn_frcnn *p, int depth, TrainState *t) {
  const int n_conv = (int)p->conv.size(), Kmax = conv_layers_above_last_pool(p);
  int k = depth > MPN_TRAIN_FC6 ? depth - MPN_TRAIN_FC6 : 0;
  if (depth >= MPN_TRAIN_TRUNK(0)) {  // k <= K: no pooling layer among them, MPN_TRAIN_CONV(k) — the same code, the same bits; k > K: pooling layers among the trained ones
    const int lim = std::min(n_conv - 1, (int)MPN_TRAIN_MAX_TRUNK);
    k = depth - MPN_TRAIN_TRUNK(0);
    if (k < 1 || k > lim) {
      set_error("mpn_frcnn_train_begin: depth %d = MPN_TRAIN_TRUNK(%d), but k runs from 1 to %d on this trunk of %d conv layers: min(n_conv - 1, MPN_TRAIN_MAX_TRUNK = %d) — the first conv layer is never trained (its input is the image)",
                depth, k, lim, n_conv, (int)MPN_TRAIN_MAX_TRUNK);
      return MPN_EINVAL;
    }
  } else if (depth > MPN_TRAIN_CONV(Kmax)) {
    set_error("mpn_frcnn_train_begin: depth %d = MPN_TRAIN_CONV(%d), but only K = %d conv layers lie above the trunk's last pooling layer: a pooling layer is in the way (it has no backward pass)",
              depth, depth - MPN_TRAIN_FC6, Kmax);
    return MPN_EINVAL;
  }
  t->n_fc = 1 + (depth >= MPN_TRAIN_FC7) + (depth >= MPN_TRAIN_FC6);
  t->kconv = k; t->first = n_conv - k;
  return MPN_OK;
}

// Where the conv block's saved maps lie in an image's slot of `acts` (act_off, pool_off, act_img), each at its own layer's size for a
// max_h x max_w input, and the size of a gradient map: the largest of the saved maps' sizes (and the final map's)
static void layout_train_maps(const mpn_frcnn *p, ConvBlock *t) {
  const mpn_frcnn_config &c = p->cfg;
  const int k = t->kconv;
  int mh = c.max_h, mw = c.max_w;
  final_map_size(p, &mh, &mw);
  size_t off = 0;
  t->gmap_bytes = act_bytes(p->feat_c, mh, mw);
  auto slot = [&](const Act &a) { const size_t b = act_bytes(a.C, a.H, a.W); off += b / sizeof(float); t->gmap_bytes = std::max(t->gmap_bytes, b); };
  for (int j = 0; j <= k; ++j) {  // map 0: the block's input; map j: the output of conv[first + j - 1], each at its own layer's size
    t->act_off[j] = off;
    slot(train_map(p, t, nullptr, j, false, c.max_h, c.max_w));
  }
  for (int j = 1; j < k; ++j) {   // MPN_TRAIN_TRUNK: the pooled map of a pooled layer is the next trained layer's input
    if (!p->conv[t->first + j - 1].pool) continue;
    t->pool_off[j] = off;
    slot(train_map(p, t, nullptr, j, true, c.max_h, c.max_w));
  }
  t->act_img = off;
}

static bool alloc_conv_block(const mpn_frcnn *p, ConvBlock *t, DeviceOwner &own);
// The Linear layers' table, every buffer of the state and (kconv > 1, on the NULL stream) the input gradient's weight forms.
// false: something failed (t's DeviceOwner holds what was made)
static bool alloc_train_state(const mpn_frcnn *p, TrainState *t) {
  const mpn_frcnn_config &c = p->cfg;
  const int F = c.fc_dim, k = t->kconv, PP = c.pooled_h * c.pooled_w;
  const size_t M = (size_t)c.max_rois, rec = (size_t)p->Mp * 8 * sizeof(float);
  t->fc[0] = LinT{p->w6, p->b6, p->K6, F, PP, 1};
  t->fc[1] = LinT{p->w7, p->b7, F, F, 1, 1};
  t->fc[2] = LinT{p->wh, p->bh, F, plain_head_width(p), 1, 0};
  auto alloc0 = [&](float **q, size_t bytes) -> bool { return t->own.alloc(q, bytes, true) == MPN_OK; };
  auto trained = [&](LinT &L) {  // momentum and the gradient at the output
    return alloc_momentum(t->own, L) && alloc0(&L.g, (size_t)(lin_np(L.N) / 8) * rec);
  };
  bool ok = trained(t->fc[2]);
  ok = ok && alloc0(&t->fc[0].x, (size_t)(round_up(p->K6, 64) / 8) * rec);
  for (int i = 1; i < 3; ++i) ok = ok && alloc0(&t->fc[i].x, (size_t)(lin_np(t->fc[i - 1].N) / 8) * rec);  // the output of the layer below
  ok = ok && alloc0(&t->head, M * plain_head_width(p) * sizeof(float));
  for (int i = 1; i >= 3 - t->n_fc; --i) ok = ok && trained(t->fc[i]);
  for (int i = 0; i < 2; ++i) { t->fc[i].y = t->fc[i + 1].x; t->fc[i].drop = i; t->fc[i + 1].dx = t->fc[i].g; }  // (dx: null below the lowest trained layer)
  t->fc[2].y_rm = t->head;
  ok = ok && alloc_core(p, *t);
  if (!k) return ok;
  ok = ok && alloc0(&t->dx6, (size_t)(round_up(p->K6, 64) / 8) * rec) && alloc0(&t->prois, M * 5 * sizeof(float));
  ok = ok && t->own.alloc(&t->argmax, M * p->feat_c * PP * sizeof(int32_t), true) == MPN_OK;
  return ok && alloc_conv_block(p, t, t->own);
}

// The conv block's buffers for its kconv > 0 layers: the images' saved maps, the two gradient maps, per layer momentum, gradient sums
// and (on the NULL stream) the input gradient's weight forms.  false: something failed (`own` holds what was made)
static bool alloc_conv_block(const mpn_frcnn *p, ConvBlock *t, DeviceOwner &own) {
  const mpn_frcnn_config &c = p->cfg;
  const int k = t->kconv;
  auto alloc0 = [&](float **q, size_t bytes) -> bool { return own.alloc(q, bytes, true) == MPN_OK; };
  layout_train_maps(p, t);
  bool ok = alloc0(&t->acts, t->act_img * MPN_TRAIN_MAX_IMAGES * sizeof(float));
  ok = ok && alloc0(&t->gmap[0], t->gmap_bytes) && alloc0(&t->gmap[1], t->gmap_bytes);
  size_t wmax = 0, pmax = 0;
  t->cl.resize(k);
  for (int j = 0; j < k && ok; ++j) {
    const ConvLayer &L = p->conv[t->first + j];
    ConvT &T = t->cl[j];
    const size_t we = conv_wpk_elems(L.Cin, L.Cout) * sizeof(float), be = (size_t)conv_coutp(L.Cout) * sizeof(float);
    ok = alloc0(&T.v, we) && alloc0(&T.vb, be) && alloc0(&T.dw, we) && alloc0(&T.db, be);
    if (j > 0) {  // a trained layer lies below: this layer hands a gradient down
      ok = ok && alloc0(&T.wpk_t, conv_wpk_elems(L.Cout, L.Cin) * sizeof(float)) && alloc0(&T.zero_b, (size_t)conv_coutp(L.Cin) * sizeof(float));
      if (t->dgrad_wino && L.Cout >= 16) ok = ok && alloc0(&T.wino_t, conv_wino_elems(L.Cout, L.Cin) * sizeof(float));
    }
    wmax = std::max(wmax, (size_t)L.Cout * L.Cin * 9);
    int lh, lw;
    layer_map_size(p, t->first + j, c.max_h, c.max_w, &lh, &lw);
    pmax = std::max(pmax, conv_wgrad_part_elems(L.Cin, L.Cout, lh, lw));
  }
  ok = ok && alloc0(&t->wtmp, 2 * wmax * sizeof(float)) && alloc0(&t->part, pmax * sizeof(float));
  for (int j = 1; j < k && ok; ++j) ok = refresh_conv_forms(p->conv[t->first + j], t->cl[j], t->wtmp, false, nullptr) == MPN_OK;
  return ok;
}

extern "C" int mpn_frcnn_train_begin(mpn_frcnn *p, int depth, float momentum, float weight_decay, float bbox_weight) {
  MPN_CHECK_ARG(p != nullptr);
  int rc = begin_refusals(p, false, __func__);
  if (rc) return rc;
  MPN_CHECK_ARG(depth >= MPN_TRAIN_HEADS);
  std::unique_ptr<TrainState> t(new TrainState());  // (its DeviceOwner gives back what a failed attempt made)
  rc = parse_train_depth(p, depth, t.get());
  if (rc == MPN_OK) rc = begin_core(*t, __func__, momentum, weight_decay, bbox_weight);
  if (rc) return rc;
  if (!alloc_train_state(p, t.get()) || hipDeviceSynchronize() != hipSuccess) {
    set_error("mpn_frcnn_train_begin: allocating the momentum / gradient buffers failed: %s", hipGetErrorString(hipGetLastError()));
    return MPN_ENOMEM;
  }
  p->train = t.release();  // all or nothing, as in mpn_frcnn_set_augment: published last, its presence says that every buffer exists
  return MPN_OK;
}

extern "C" int mpn_frcnn_train_end(mpn_frcnn *p) {
  MPN_CHECK_ARG(p != nullptr);
  return train_end(p, false, __func__);
}

// ---- drawing an image's rows on the device (*_train_add_sampled; sampler.h) ----
// the sampled-row buffers for `rows` rows (train_begin made them for max_rois rows; a larger batch_size regrows them)
static int grow_sample_rows(SampleBufs &b, DeviceOwner &own, size_t rows, hipStream_t s) {
  int rc = own.grow(&b.rois, &b.rois_b, rows * 4 * sizeof(float), s);
  if (rc == MPN_OK) rc = own.grow(&b.gt, &b.gt_b, rows * 4 * sizeof(float), s);
  if (rc == MPN_OK) rc = own.grow(&b.labels, &b.labels_b, rows * sizeof(int), s);
  return rc;
}

// The refusals of the sampled entry points' own arguments (the handle's state has been checked), before any launch
static int check_sampled_args(const char *fn, const float *d_image, int H0, int W0, const float *d_proposals, int n, const float *d_gt,
                              const int *d_gt_labels, int g, const float *d_crowds, int n_crowd, const mpn_roi_sampler *cfg, const int *h_counts) {
  if (!d_image || !h_counts || H0 <= 0 || W0 <= 0) {
    set_error("%s: invalid argument: %s", fn, !d_image ? "d_image is NULL" : !h_counts ? "h_counts is NULL" : "H <= 0 or W <= 0");
    return MPN_EINVAL;
  }
  int rc = check_attach_args(fn, d_proposals, n, d_gt, d_gt_labels, g, d_crowds, n_crowd);
  if (rc == MPN_OK) rc = check_sampler_cfg(fn, cfg, 0);
  return rc;
}

// Attach and sample one image into b (both launches on s), then the two counts back into h_counts: one stream synchronisation, after
// which the caller knows how many rows the image gives before the trunk runs.  flip_width > 0: the sampled boxes flipped at that width.
static int sample_image(SampleBufs &b, DeviceOwner &own, const float *d_proposals, int n, const float *d_gt, const int *d_gt_labels, int g,
                        const float *d_crowds, int n_crowd, const mpn_roi_sampler &cfg, uint64_t seed, uint64_t draw, int flip_width,
                        int *h_counts, hipStream_t s) {
  const size_t m = (size_t)g + n;
  int rc = grow_sample_rows(b, own, std::min((size_t)cfg.batch_size, 2 * m), s);  // r_bg <= n_bg <= m, r_fg <= n_fg <= m
  if (rc == MPN_OK) rc = own.grow(&b.boxes, &b.boxes_b, m * 4 * sizeof(float), s);
  if (rc == MPN_OK) rc = own.grow(&b.overlap, &b.overlap_b, m * sizeof(float), s);
  if (rc == MPN_OK) rc = own.grow(&b.corr, &b.corr_b, m * sizeof(int), s);
  if (rc == MPN_OK) rc = own.grow(&b.label, &b.label_b, m * sizeof(int), s);
  if (rc == MPN_OK) rc = own.grow(&b.lists, &b.lists_b, 2 * m * sizeof(int), s);
  if (rc == MPN_OK) rc = attach_proposals(d_proposals, n, d_gt, d_gt_labels, g, d_crowds, n_crowd, b.boxes, b.overlap, b.corr, b.label, s);
  if (rc == MPN_OK) rc = roi_sample(b.boxes, b.overlap, b.corr, b.label, (int)m, cfg, seed, draw, flip_width, b.lists, b.rois, b.gt, b.labels, b.counts, s);
  if (rc) return rc;
  MPN_CHECK_HIP(hipMemcpyAsync(h_counts, b.counts, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
  MPN_CHECK_HIP(hipStreamSynchronize(s));
  return MPN_OK;
}

// rows the sampler wrote for these counts, both >= 1: r_bg + r_fg >= 1, as batch_size >= 1 gives one of the two sets a quota
static int sampled_rows(const mpn_roi_sampler &cfg, const int *counts) {
  const int fg_num = sampler_fg_num(cfg);
  return std::min(cfg.batch_size - fg_num, counts[0]) + std::min(fg_num, counts[1]);
}

// the image of a flipped add: mpn_image_hflip's kernel into the state's own buffer
static int flip_train_image(SampleBufs &b, DeviceOwner &own, const float *d_image, int H0, int W0, hipStream_t s, const float **d_out) {
  int rc = own.grow(&b.flipped, &b.flipped_b, (size_t)3 * H0 * W0 * sizeof(float), s);
  if (rc == MPN_OK) rc = mpn_image_hflip(d_image, 3, H0, W0, b.flipped, s);
  *d_out = b.flipped;
  return rc;
}

// What one more image of n rows behind the pending ones must satisfy (the four *_train_add* entry points, under the caller's name `fn`),
// and getImages' size
static int add_check(mpn_frcnn *p, bool mpnet, const char *fn, int H0, int W0, int n, double *sc, int *H, int *W) {
  const mpn_frcnn_config &c = p->cfg;
  const int pending = core_of(p, mpnet)->pending;
  if (pending + n > c.max_rois) {
    set_error("%s: %d pending rows + %d exceed the handle's max_rois (%d)", fn, pending, n, c.max_rois);
    return MPN_EINVAL;
  }
  *sc = 1.0; *H = H0; *W = W0;
  if (c.scale_target > 0.0) *sc = getimages_size(H0, W0, c.scale_target, c.scale_max, H, W);
  if (*H <= 0 || *W <= 0 || *H > c.max_h || *W > c.max_w) {
    set_error("%s: %dx%d image (scaled to %dx%d) exceeds the pipeline's %dx%d", fn, H0, W0, *H, *W, c.max_h, c.max_w);
    return MPN_EINVAL;
  }
  const ConvBlock *t = mpnet ? static_cast<const ConvBlock *>(p->tower_train) : p->train;
  if (t && t->kconv && t->n_img >= MPN_TRAIN_MAX_IMAGES) {
    set_error("%s: %d images are pending: a step %s takes at most MPN_TRAIN_MAX_IMAGES = %d images", fn, t->n_img,
              mpnet ? "that trains conv layers (mpn_mpnet_train_begin_conv, k > 0)" : "at depth MPN_TRAIN_CONV(k)", MPN_TRAIN_MAX_IMAGES);
    return MPN_EINVAL;
  }
  return MPN_OK;
}

// the kinds' bodies of an add on device row pointers, everything checked (below): the frozen trunk, the kind's ROI pooling, the rows' copies
static int frcnn_add_rows(mpn_frcnn *p, TrainState *t, const float *d_image, int H0, int W0, int H, int W, double sc, const float *d_rois,
                          const float *d_gt, const int *d_labels, int n, hipStream_t s);
static int mpnet_add_rows(mpn_frcnn *p, TowerTrainState *t, const float *d_image, int H0, int W0, int H, int W, double sc, const float *d_rois,
                          const float *d_gt, const int *d_labels, int n, hipStream_t s);
static int add_rows(mpn_frcnn *p, bool mpnet, const float *d_image, int H0, int W0, int H, int W, double sc, const float *d_rois, const float *d_gt,
                    const int *d_labels, int n, hipStream_t s) {
  return mpnet ? mpnet_add_rows(p, p->tower_train, d_image, H0, W0, H, W, sc, d_rois, d_gt, d_labels, n, s)
               : frcnn_add_rows(p, p->train, d_image, H0, W0, H, W, sc, d_rois, d_gt, d_labels, n, s);
}
// ... which both end with the rows' copies behind the pending ones (fn: the kind's body)
static int append_rows(TrainCore &c, const char *fn, const float *d_rois, const float *d_gt, const int *d_labels, int n, hipStream_t s) {
  CHECK_HIP_AS(fn, hipMemcpyAsync(c.rois + (size_t)c.pending * 4, d_rois, (size_t)n * 4 * sizeof(float), hipMemcpyDeviceToDevice, s));
  CHECK_HIP_AS(fn, hipMemcpyAsync(c.gt + (size_t)c.pending * 4, d_gt, (size_t)n * 4 * sizeof(float), hipMemcpyDeviceToDevice, s));
  CHECK_HIP_AS(fn, hipMemcpyAsync(c.labels + c.pending, d_labels, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, s));
  c.pending += n;
  return MPN_OK;
}

// mpn_frcnn_train_add and mpn_mpnet_train_add behind their `p != nullptr`
static int train_add(mpn_frcnn *p, bool mpnet, const char *fn, const float *d_image, int H0, int W0, const float *d_rois, const float *d_gt,
                     const int *d_labels, int n, void *stream) {
  int rc = refuse_train(p, mpnet, fn);
  if (rc) return rc;
  TrainCore *t;
  if ((rc = need_core(p, mpnet, fn, &t)) != MPN_OK) return rc;
  CHECK_ARG_AS(fn, d_image && d_rois && d_gt && d_labels && n > 0 && H0 > 0 && W0 > 0);
  double sc;
  int H, W;
  if ((rc = add_check(p, mpnet, fn, H0, W0, n, &sc, &H, &W)) != MPN_OK) return rc;
  ScratchScope scratch_scope(&p->scratch);
  return add_rows(p, mpnet, d_image, H0, W0, H, W, sc, d_rois, d_gt, d_labels, n, as_stream(stream));
}

// ... and the two *_train_add_sampled
static int train_add_sampled(mpn_frcnn *p, bool mpnet, const char *fn, const float *d_image, int H0, int W0, const float *d_proposals, int n,
                             const float *d_gt, const int *d_gt_labels, int g, const float *d_crowds, int n_crowd, const mpn_roi_sampler *cfg,
                             uint64_t seed, uint64_t draw, int flip, int *h_counts, void *stream) {
  int rc = refuse_train(p, mpnet, fn);
  if (rc) return rc;
  TrainCore *t;
  if ((rc = need_core(p, mpnet, fn, &t)) != MPN_OK) return rc;
  if ((rc = check_sampled_args(fn, d_image, H0, W0, d_proposals, n, d_gt, d_gt_labels, g, d_crowds, n_crowd, cfg, h_counts)) != MPN_OK) return rc;
  ScratchScope scratch_scope(&p->scratch);
  hipStream_t s = as_stream(stream);
  rc = sample_image(t->smp, t->own, d_proposals, n, d_gt, d_gt_labels, g, d_crowds, n_crowd, *cfg, seed, draw, flip ? W0 : 0, h_counts, s);
  if (rc) return rc;
  if (h_counts[0] == 0 || h_counts[1] == 0) return MPN_OK;  // no background or no foreground: nothing is added, the caller draws another image
  const int r = sampled_rows(*cfg, h_counts);
  double sc;
  int H, W;
  if ((rc = add_check(p, mpnet, fn, H0, W0, r, &sc, &H, &W)) != MPN_OK) return rc;
  if (flip && (rc = flip_train_image(t->smp, t->own, d_image, H0, W0, s, &d_image)) != MPN_OK) return rc;
  return add_rows(p, mpnet, d_image, H0, W0, H, W, sc, t->smp.rois, t->smp.gt, t->smp.labels, r, s);
}

extern "C" int mpn_frcnn_train_add(mpn_frcnn *p, const float *d_image, int H0, int W0, const float *d_rois, const float *d_gt,
                                   const int *d_labels, int n, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  return train_add(p, false, __func__, d_image, H0, W0, d_rois, d_gt, d_labels, n, stream);
}
extern "C" int mpn_mpnet_train_add(mpn_frcnn *p, const float *d_image, int H0, int W0, const float *d_rois, const float *d_gt, const int *d_labels,
                                   int n, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  return train_add(p, true, __func__, d_image, H0, W0, d_rois, d_gt, d_labels, n, stream);
}
extern "C" int mpn_frcnn_train_add_sampled(mpn_frcnn *p, const float *d_image, int H0, int W0, const float *d_proposals, int n, const float *d_gt,
                                           const int *d_gt_labels, int g, const float *d_crowds, int n_crowd, const mpn_roi_sampler *cfg,
                                           uint64_t seed, uint64_t draw, int flip, int *h_counts, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  return train_add_sampled(p, false, __func__, d_image, H0, W0, d_proposals, n, d_gt, d_gt_labels, g, d_crowds, n_crowd, cfg, seed, draw, flip, h_counts, stream);
}
extern "C" int mpn_mpnet_train_add_sampled(mpn_frcnn *p, const float *d_image, int H0, int W0, const float *d_proposals, int n, const float *d_gt,
                                           const int *d_gt_labels, int g, const float *d_crowds, int n_crowd, const mpn_roi_sampler *cfg,
                                           uint64_t seed, uint64_t draw, int flip, int *h_counts, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  return train_add_sampled(p, true, __func__, d_image, H0, W0, d_proposals, n, d_gt, d_gt_labels, g, d_crowds, n_crowd, cfg, seed, draw, flip, h_counts, stream);
}

// What the conv block's backward pass reads of the image whose trunk pass has just run (final map `feat`, network input H x W), into
// the next image slot: the block's input map, every trained layer's output, and the image's record — its n rows start at row0
static int save_conv_maps(mpn_frcnn *p, ConvBlock *t, const Act &feat, int H, int W, int row0, int n, hipStream_t s) {
  const int i = t->n_img, k = t->kconv;
  float *slot = t->acts + (size_t)i * t->act_img;
  for (int j = 0; j <= k; ++j) {
    const ConvLayer &L = p->conv[t->first + j - 1];   // j == 0: the layer below the trained ones
    // j == 0: what conv[first] read; j >= 1: the layer's output before its pool (the last layer's unpooled output is the final map)
    const float *src = j == 0 ? (L.pool ? L.pooled : L.out) : ((j == k && !L.pool) ? feat.p : L.out);
    const Act a = train_map(p, t, slot, j, false, H, W);
    MPN_CHECK_HIP(hipMemcpyAsync(a.p, src, act_bytes(a.C, a.H, a.W), hipMemcpyDeviceToDevice, s));
    if (j >= 1 && j < k && L.pool) {
      const Act ap = train_map(p, t, slot, j, true, H, W);
      MPN_CHECK_HIP(hipMemcpyAsync(ap.p, L.pooled, act_bytes(ap.C, ap.H, ap.W), hipMemcpyDeviceToDevice, s));
    }
  }
  t->img_h[i] = feat.H; t->img_w[i] = feat.W; t->img_nh[i] = H; t->img_nw[i] = W; t->img_row0[i] = row0; t->img_rows[i] = n;
  ++t->n_img;
  return MPN_OK;
}

// The plain handle's add: the frozen trunk, the ROI pooling of these rows behind the pending ones, what the conv block's backward pass
// reads, the rows' copies
static int frcnn_add_rows(mpn_frcnn *p, TrainState *t, const float *d_image, int H0, int W0, int H, int W, double sc, const float *d_rois,
                          const float *d_gt, const int *d_labels, int n, hipStream_t s) {
  const mpn_frcnn_config &c = p->cfg;
  int rc = MPN_OK;
  p->seg_shape[0][0] = -1;  // (as run_detect) the trunk's buffers and the ROI table are rewritten: the next head segment runs for real
  Act feat;
  bool pools = false;  // a pooled layer among the trained ones (MPN_TRAIN_TRUNK): this trunk pass also writes their pre-pool maps
  for (int j = 0; j < t->kconv; ++j) pools = pools || p->conv[t->first + j].pool;
  if (pools) p->keep_prepool_from = t->first;
  rc = obtain_features(p, d_image, H0, W0, H, W, sc, &p->up, s, &feat);  // getImages' rescale + the frozen trunk, exactly as detect
  p->keep_prepool_from = -1;
  // the map now belongs to a training image: nothing a detect on cached features may pool from
  p->up.invalidate(); p->mir.invalidate();
  if (rc) return rc;
  rc = mpn_project_im_rois(d_rois, n, sc, p->rois, s);
  if (rc) return rc;
  // this image's rows behind the pending ones: a shifted base pointer with the buffer's row pitch
  rc = roi_pool_c8(feat, p->rois, n, c.pooled_h, c.pooled_w, c.spatial_scale, RoiRule{1.0f, 0, c.roi_bin_rule}, t->fc[0].x + (size_t)t->pending * 8,
                   t->kconv ? t->argmax + (size_t)t->pending * p->feat_c * c.pooled_h * c.pooled_w : nullptr, s, 5, p->Mp);
  if (rc) return rc;
  if (t->kconv) {  // what the conv block's backward pass reads: the block's input, every trained layer's output, the rows' windows
    MPN_CHECK_HIP(hipMemcpyAsync(t->prois + (size_t)t->pending * 5, p->rois, (size_t)n * 5 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if ((rc = save_conv_maps(p, t, feat, H, W, t->pending, n, s)) != MPN_OK) return rc;
  }
  return append_rows(*t, __func__, d_rois, d_gt, d_labels, n, s);
}

// The conv block's backward pass for image i from where its gradient map is laid: G = the gradient at the last trained layer's output
// (masked with that layer's ReLU) in gmap[cur], a zero-haloed map, the other gradient map zeroed too.  Last trained layer to first:
// the bias and weight gradients (added to the step's sums from the second image on) and the input gradient masked with the ReLU of the
// layer below.  No weight is touched.  Both kinds' steps end in it.
static int conv_chain_backward(mpn_frcnn *p, ConvBlock *t, int i, Act G, int cur, hipStream_t s) {
  const int nh = t->img_nh[i], nw = t->img_nw[i], k = t->kconv;
  float *slot = t->acts + (size_t)i * t->act_img;
  bool relaid = false;  // a pooling layer has been crossed: the caller's memset no longer is the halo of the maps' sizes
  int rc = MPN_OK;
  for (int j = k; j >= 1 && rc == MPN_OK; --j) {
    const ConvLayer &L = p->conv[t->first + j - 1];
    const ConvT &T = t->cl[j - 1];
    const Act X = train_in_map(p, t, slot, j, nh, nw);
    if (L.pool) {  // G is the gradient at the pooled output: route it to the pre-pool map's maxima, masked with that map's ReLU
      const Act Y = train_map(p, t, slot, j, false, nh, nw);
      Act Gl = make_act(t->gmap[cur ^ 1], L.Cout, Y.H, Y.W);
      rc = c8p_zero_halos(&Gl, 1, s);
      if (rc == MPN_OK) rc = maxpool2x2_backward_c8p(Y, G, Gl, 1, s);
      if (rc != MPN_OK) break;
      G = Gl; cur ^= 1; relaid = true;
    }
    rc = conv_bias_grad(G, T.db, i > 0, s);
    if (rc == MPN_OK) rc = conv3x3_wgrad(X, G, t->part, T.dw, i > 0, s);
    if (rc != MPN_OK || j == 1) break;
    Act dX = make_act(t->gmap[cur ^ 1], L.Cin, X.H, X.W);
    if (relaid) rc = c8p_zero_halos(&dX, 1, s);
    if (rc == MPN_OK) rc = conv3x3_c8p(G, T.wpk_t, T.zero_b, L.Cin, 0, dX, Act{}, s, T.wino_t);
    if (rc == MPN_OK && !p->conv[t->first + j - 2].pool) rc = relu_mask_c8p(dX, X, s);  // (a pooled layer below: its pool's backward masks)
    G = dX; cur ^= 1;
  }
  return rc;
}

// optim.sgd on the block's layers behind a step's backward pass: the master `wpk` in place, then every form derived from it; the
// pending images become the last step's
static int conv_block_update(mpn_frcnn *p, ConvBlock *t, const TrainCore &c, float lr, int rc, hipStream_t s) {
  for (int j = 0; j < t->kconv && rc == MPN_OK; ++j) {
    const ConvLayer &L = p->conv[t->first + j];
    const ConvT &T = t->cl[j];
    rc = conv_sgd(L.wpk, T.v, T.dw, L.Cin, L.Cout, lr, c.momentum, c.weight_decay, s);
    if (rc == MPN_OK) rc = vec_sgd(L.bpk, T.vb, T.db, L.Cout, lr, c.momentum, s);
    if (rc == MPN_OK) rc = refresh_conv_forms(L, T, t->wtmp, true, s);
  }
  t->last_img = t->n_img; t->n_img = 0;
  return rc;
}

// The backward pass below fc6 (depth MPN_TRAIN_CONV(k)): the gradient at the pooled features, then per image — in train_add order — the
// ROI-pooling backward into a zero-haloed gradient map and conv_chain_backward: last trained layer to first, the bias and weight gradients
// (added to the step's sums) and the input gradient masked with the ReLU of the layer below.  No weight is touched: the caller updates
// afterwards.  MPN_TRAIN_TRUNK(k): every layer at its own size; at a pooled layer the gradient at its pooled output first goes through
// maxpool2x2_backward_c8p (fused with the ReLU mask of the pre-pool map, so the input gradient handed to a pooled layer is not masked
// on its own) into the other gradient map, whose halo is laid for the larger size first — as is every map written after it.
static int train_conv_backward(mpn_frcnn *p, TrainState *t, int B, hipStream_t s) {
  const mpn_frcnn_config &c = p->cfg;
  const int PP = c.pooled_h * c.pooled_w, Mp = p->Mp;
  // dx6 = (g6 W6) .* [x6 > 0]: fc6's packed chunk order is x6's.  The mask is the last conv layer's ReLU mask (pooled values are map values)
  const LinT &L6 = t->fc[0];
  int rc = linear_dgrad_c8(L6.g, Mp, B, L6.N, L6.w, L6.K, L6.x, t->dx6, Mp, s);
  for (int i = 0; i < t->n_img && rc == MPN_OK; ++i) {
    const int h = t->img_h[i], w = t->img_w[i];
    for (float *gm : t->gmap) MPN_CHECK_HIP(hipMemsetAsync(gm, 0, t->gmap_bytes, s));  // the halo is the input gradient's padding
    int cur = 0;
    Act G = make_act(t->gmap[cur], p->feat_c, h, w);
    RoiBwd a{};
    a.g = t->dx6; a.argmax = t->argmax; a.rois = t->prois; a.by_batch = 0; a.n0 = t->img_row0[i]; a.n1 = a.n0 + t->img_rows[i];
    a.B = 1; a.C = p->feat_c; a.H = h; a.W = w; a.PH = c.pooled_h; a.PW = c.pooled_w; a.windows = (c.pooled_h <= 32 && c.pooled_w <= 32) ? 1 : 0;
    a.g_n = 8; a.g_cb = (long)PP * Mp * 8; a.g_c = 1; a.g_bin = (long)Mp * 8;
    a.o_b = 0; a.o_cb = (long)G.plane(); a.o_c = 1; a.o_y = (long)G.Wp * 8; a.o_x = 8;
    a.scale = c.spatial_scale; a.rr = RoiRule{1.0f, 0, c.roi_bin_rule};
    a.out = G.p + ((size_t)G.Wp + 1) * 8;
    rc = roi_pool_backward(a, s);
    if (rc == MPN_OK) rc = conv_chain_backward(p, t, i, G, cur, s);
  }
  return rc;
}

// A step up to its first launch: the kind's refusals, a begun state with pending rows, a finite rate.  *step: this step's masks —
// counted whatever the rate, also when a launch fails
static int step_begin(mpn_frcnn *p, bool mpnet, const char *fn, float lr, TrainCore **c, long *step) {
  int rc = refuse_train(p, mpnet, fn);
  if (rc == MPN_OK) rc = need_core(p, mpnet, fn, c);
  if (rc) return rc;
  if ((*c)->pending <= 0) { set_error("%s: no pending rows (%s_train_add first)", fn, kind_prefix(mpnet)); return MPN_ESTATE; }
  CHECK_ARG_AS(fn, std::isfinite(lr));
  *step = (*c)->step++;
  return MPN_OK;
}
// ... and behind its last one (also a failed one: the weights may be half updated, the batch is not to be replayed)
static void step_end(TrainCore &c) {
  c.last_rows = c.pending;
  c.pending = 0;
}

static const int kPlainBwd[3] = {2, 1, 0};  // head, fc7, fc6

extern "C" int mpn_frcnn_train_step(mpn_frcnn *p, float lr, float *d_loss, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  TrainCore *core;
  long step;
  int rc = step_begin(p, false, __func__, lr, &core, &step);
  if (rc) return rc;
  TrainState *t = static_cast<TrainState *>(core);
  const int B = t->pending, Mp = p->Mp;
  ScratchScope scratch_scope(&p->scratch);
  hipStream_t s = as_stream(stream);
  rc = lin_forward(t->fc, 3, *t, B, Mp, step, s);  // the last layer writes the row-major head
  if (rc) return rc;
  rc = train_loss(t->head, B, p->cfg.n_classes, p->n_integral, t->head_k, t->rois, t->gt, t->labels, loss_cfg(p, *t), t->fc[2].g, Mp, d_loss ? d_loss : t->loss, s);
  if (rc == MPN_OK) rc = lin_dgrad(t->fc, kPlainBwd, 3, *t, B, Mp, s);  // down to the lowest trained layer
  if (rc == MPN_OK && t->kconv) rc = train_conv_backward(p, t, B, s);
  if (rc == MPN_OK) rc = lin_update(t->fc, kPlainBwd, 3, *t, B, Mp, lr, nullptr, s);
  rc = conv_block_update(p, t, *t, lr, rc, s);
  step_end(*t);
  return rc;
}

extern "C" int mpn_frcnn_train_set_head(mpn_frcnn *p, int k) {
  MPN_CHECK_ARG(p != nullptr);
  return train_set_head(p, false, __func__, k);
}
extern "C" int mpn_mpnet_train_set_head(mpn_frcnn *p, int k) {
  MPN_CHECK_ARG(p != nullptr);
  return train_set_head(p, true, __func__, k);
}
extern "C" int mpn_frcnn_train_set_dropout(mpn_frcnn *p, float rate, long seed) {
  MPN_CHECK_ARG(p != nullptr);
  return train_set_dropout(p, false, __func__, rate, seed);
}
extern "C" int mpn_mpnet_train_set_dropout(mpn_frcnn *p, float rate, long seed) {
  MPN_CHECK_ARG(p != nullptr);
  return train_set_dropout(p, true, __func__, rate, seed);
}

// The eight tensors of mpn_frcnn_train_get_state / _set_state in their order, each with the Linear layer whose momentum holds it
namespace {
struct StateTensor { const char *name; int fc; };
const StateTensor kStateTensors[8] = {{"d_fc6_v", 0}, {"d_fc6_vb", 0}, {"d_fc7_v", 1}, {"d_fc7_vb", 1}, {"d_cls_v", 2}, {"d_cls_vb", 2}, {"d_bbox_v", 2}, {"d_bbox_vb", 2}};
}
// a tensor of a layer the depth does not train has no momentum: it must be NULL
static int check_state_tensors(const TrainState *t, const char *fn, const float *const q[8], bool need_all) {
  for (int i = 0; i < 8; ++i) {
    const bool trained = kStateTensors[i].fc >= 3 - t->n_fc;
    if (q[i] && !trained) {
      set_error("%s: %s must be NULL: this training depth does not train that tensor (it has no momentum)", fn, kStateTensors[i].name);
      return MPN_EINVAL;
    }
    if (!q[i] && trained && need_all) {
      set_error("%s: %s is NULL, but this training depth trains that tensor: its momentum is part of the state", fn, kStateTensors[i].name);
      return MPN_EINVAL;
    }
  }
  return MPN_OK;
}

extern "C" int mpn_frcnn_train_get_state(mpn_frcnn *p, float *d_fc6_v, float *d_fc6_vb, float *d_fc7_v, float *d_fc7_vb, float *d_cls_v,
                                         float *d_cls_vb, float *d_bbox_v, float *d_bbox_vb, long *h_step, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  const TrainState *t = p->train;
  if (!t) { set_error("mpn_frcnn_train_get_state: no mpn_frcnn_train_begin on this handle"); return MPN_ESTATE; }
  const float *const q[8] = {d_fc6_v, d_fc6_vb, d_fc7_v, d_fc7_vb, d_cls_v, d_cls_vb, d_bbox_v, d_bbox_vb};
  int rc = check_state_tensors(t, "mpn_frcnn_train_get_state", q, false);
  if (rc) return rc;
  const int KC = p->n_integral * p->cfg.n_classes;  // the K classifiers' rows of the fused head, bbox behind them
  hipStream_t s = as_stream(stream);
  for (int i = 3 - t->n_fc; i < 2 && rc == MPN_OK; ++i) {
    const LinT &L = t->fc[i];
    rc = unpack_linear_weights(L.v, L.vb, L.K, L.N, L.inner, 0, L.N, i ? d_fc7_v : d_fc6_v, i ? d_fc7_vb : d_fc6_vb, s);
  }
  const LinT &Lh = t->fc[2];
  if (rc == MPN_OK) rc = unpack_linear_weights(Lh.v, Lh.vb, Lh.K, Lh.N, 1, 0, KC, d_cls_v, d_cls_vb, s);
  if (rc == MPN_OK) rc = unpack_linear_weights(Lh.v, Lh.vb, Lh.K, Lh.N, 1, KC, Lh.N, d_bbox_v, d_bbox_vb, s);
  if (rc == MPN_OK && h_step) *h_step = t->step;
  return rc;
}

extern "C" int mpn_frcnn_train_set_state(mpn_frcnn *p, const float *d_fc6_v, const float *d_fc6_vb, const float *d_fc7_v, const float *d_fc7_vb,
                                         const float *d_cls_v, const float *d_cls_vb, const float *d_bbox_v, const float *d_bbox_vb, long step,
                                         void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  TrainState *t = p->train;
  if (!t) { set_error("mpn_frcnn_train_set_state: no mpn_frcnn_train_begin on this handle"); return MPN_ESTATE; }
  if (t->pending > 0) { set_error("mpn_frcnn_train_set_state: %d rows are pending: take the step (mpn_frcnn_train_step) first", t->pending); return MPN_ESTATE; }
  const float *const q[8] = {d_fc6_v, d_fc6_vb, d_fc7_v, d_fc7_vb, d_cls_v, d_cls_vb, d_bbox_v, d_bbox_vb};
  int rc = check_state_tensors(t, "mpn_frcnn_train_set_state", q, true);
  if (rc) return rc;
  if (step < 0) { set_error("mpn_frcnn_train_set_state: step %ld is negative", step); return MPN_EINVAL; }
  const int C = p->cfg.n_classes, F = p->cfg.fc_dim, KC = p->n_integral * C, NH = plain_head_width(p);
  hipStream_t s = as_stream(stream);
  if (!t->vtmp && t->own.alloc(&t->vtmp, ((size_t)NH * F + NH) * sizeof(float), true) != MPN_OK) {
    set_error("mpn_frcnn_train_set_state: allocating the joined head momentum failed: %s", hipGetErrorString(hipGetLastError()));
    return MPN_ENOMEM;
  }
  for (int i = 3 - t->n_fc; i < 2 && rc == MPN_OK; ++i) {
    const LinT &L = t->fc[i];
    rc = pack_linear_weights(i ? d_fc7_v : d_fc6_v, i ? d_fc7_vb : d_fc6_vb, L.K, L.N, L.inner, L.v, L.vb, s);
  }
  if (rc) return rc;
  // cls (the K classifiers stacked) and bbox joined into the fused head's [(K+4)C, F] as creation joins the weights, then the same packer
  float *jw = t->vtmp, *jb = t->vtmp + (size_t)NH * F;
  MPN_CHECK_HIP(hipMemcpyAsync(jw, d_cls_v, (size_t)KC * F * sizeof(float), hipMemcpyDeviceToDevice, s));
  MPN_CHECK_HIP(hipMemcpyAsync(jw + (size_t)KC * F, d_bbox_v, (size_t)4 * C * F * sizeof(float), hipMemcpyDeviceToDevice, s));
  MPN_CHECK_HIP(hipMemcpyAsync(jb, d_cls_vb, (size_t)KC * sizeof(float), hipMemcpyDeviceToDevice, s));
  MPN_CHECK_HIP(hipMemcpyAsync(jb + KC, d_bbox_vb, (size_t)4 * C * sizeof(float), hipMemcpyDeviceToDevice, s));
  const LinT &Lh = t->fc[2];
  rc = pack_linear_weights(jw, jb, Lh.K, Lh.N, 1, Lh.v, Lh.vb, s);
  if (rc == MPN_OK) t->step = step;
  return rc;
}

// conv[layer] as a trained layer of a state's conv block: its ConvT, or a refusal naming the trained range
static int block_layer(ConvBlock *t, const char *fn, int layer, ConvT **T_out) {
  if (layer < t->first || layer >= t->first + t->kconv || !t->kconv) {
    if (t->kconv) set_error("%s: conv layer %d is not trained at this depth (layers %d .. %d are): it has no momentum", fn, layer, t->first, t->first + t->kconv - 1);
    else set_error("%s: conv layer %d is not trained at this depth (no conv layer is): it has no momentum", fn, layer);
    return MPN_EINVAL;
  }
  *T_out = &t->cl[layer - t->first];
  return MPN_OK;
}
static int trained_conv(mpn_frcnn *p, const char *fn, int layer, TrainState **t_out, ConvT **T_out) {
  TrainState *t = p->train;
  if (!t) { set_error("%s: no mpn_frcnn_train_begin on this handle", fn); return MPN_ESTATE; }
  *t_out = t;
  return block_layer(t, fn, layer, T_out);
}
// every trained conv layer's momentum, weight and bias (*_train_scale_momentum)
static int scale_conv_momentum(const mpn_frcnn *p, const ConvBlock *t, float factor, hipStream_t s) {
  int rc = MPN_OK;
  for (int j = 0; j < t->kconv && rc == MPN_OK; ++j) {
    const ConvLayer &L = p->conv[t->first + j];
    rc = scale_momentum(t->cl[j].v, conv_wpk_elems(L.Cin, L.Cout), factor, s);
    if (rc == MPN_OK) rc = scale_momentum(t->cl[j].vb, (size_t)conv_coutp(L.Cout), factor, s);
  }
  return rc;
}

extern "C" int mpn_frcnn_train_get_trunk_state(mpn_frcnn *p, int layer, float *d_v, float *d_vb, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  TrainState *t; ConvT *T;
  int rc = trained_conv(p, "mpn_frcnn_train_get_trunk_state", layer, &t, &T);
  if (rc) return rc;
  const ConvLayer &L = p->conv[layer];
  return unpack_conv_weights(T->v, T->vb, L.Cin, L.Cout, d_v, d_vb, as_stream(stream));
}

extern "C" int mpn_frcnn_train_set_trunk_state(mpn_frcnn *p, int layer, const float *d_v, const float *d_vb, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  TrainState *t; ConvT *T;
  int rc = trained_conv(p, "mpn_frcnn_train_set_trunk_state", layer, &t, &T);
  if (rc) return rc;
  if (t->pending > 0) { set_error("mpn_frcnn_train_set_trunk_state: %d rows are pending: take the step (mpn_frcnn_train_step) first", t->pending); return MPN_ESTATE; }
  if (!d_v || !d_vb) { set_error("mpn_frcnn_train_set_trunk_state: %s is NULL: a trained layer's state is its weight and its bias momentum", d_v ? "d_vb" : "d_v"); return MPN_EINVAL; }
  const ConvLayer &L = p->conv[layer];
  return pack_conv_weights(d_v, d_vb, L.Cin, L.Cout, T->v, T->vb, as_stream(stream));
}

extern "C" int mpn_frcnn_get_head_weights(mpn_frcnn *p, float *d_fc6_w, float *d_fc6_b, float *d_fc7_w, float *d_fc7_b, float *d_cls_w,
                                          float *d_cls_b, float *d_bbox_w, float *d_bbox_b, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  if (p->is_mpnet || p->rn) {
    set_error("mpn_frcnn_get_head_weights: a %s handle has no fc6 / fc7 / fused cls + bbox head to unpack", handle_kind_name(p));
    return MPN_ESTATE;
  }
  const mpn_frcnn_config &c = p->cfg;
  const int F = c.fc_dim, KC = p->n_integral * c.n_classes, NH = plain_head_width(p);  // cls: the K classifiers' rows [K*C, F]
  hipStream_t s = as_stream(stream);
  int rc = unpack_linear_weights(p->w6, p->b6, p->K6, F, c.pooled_h * c.pooled_w, 0, F, d_fc6_w, d_fc6_b, s);
  if (rc == MPN_OK) rc = unpack_linear_weights(p->w7, p->b7, F, F, 1, 0, F, d_fc7_w, d_fc7_b, s);
  if (rc == MPN_OK) rc = unpack_linear_weights(p->wh, p->bh, F, NH, 1, 0, KC, d_cls_w, d_cls_b, s);
  if (rc == MPN_OK) rc = unpack_linear_weights(p->wh, p->bh, F, NH, 1, KC, NH, d_bbox_w, d_bbox_b, s);
  return rc;
}

extern "C" int mpn_frcnn_get_trunk_weights(mpn_frcnn *p, int layer, float *d_w, float *d_b, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  if (p->is_mpnet || p->rn) {
    set_error("mpn_frcnn_get_trunk_weights: a %s handle is not supported: only mpn_frcnn_create's VGG trunk is unpacked", handle_kind_name(p));
    return MPN_ESTATE;
  }
  if (layer < 0 || layer >= (int)p->conv.size()) { set_error("mpn_frcnn_get_trunk_weights: layer %d of a %d-layer trunk", layer, (int)p->conv.size()); return MPN_EINVAL; }
  const ConvLayer &L = p->conv[layer];
  return unpack_conv_weights(L.wpk, L.bpk, L.Cin, L.Cout, d_w, d_b, as_stream(stream));
}

// =================================================================================================================================
// MultiPathNet's towers with the trunk frozen (include/mpn.h mpn_mpnet_train_*): models/multipathnet.lua
// phase 1 — the trunk inside nn.NoBackprop, everything trainable behind the ROI pooling: per tower the 1x1 mix, fc6, fc7, on top
// the K classifiers on the Foveal towers' concat and the box regressor on the het tower.  mpn_frcnn_train_* keeps refusing these
// handles (refuse_train); these entry points refuse every other kind.
// =================================================================================================================================
// The layer table and every buffer of the state; false: something failed (t's DeviceOwner holds what was made)
static bool alloc_tower_train_state(const mpn_frcnn *p, TowerTrainState *t) {
  const mpn_frcnn_config &c = p->cfg;
  const int F = c.fc_dim, PP = c.pooled_h * c.pooled_w, C = c.n_classes, KC = p->n_integral * C, c5 = p->feat_c;
  const int T = (int)p->towers.size(), nf = T - 1, Fcb = lin_np(F) / 8;
  const size_t M = (size_t)c.max_rois, rec = (size_t)p->Mp * 8 * sizeof(float), k6_rec = (size_t)(round_up(p->K6, 64) / 8) * rec;
  const size_t slice = (size_t)Fcb * p->Mp * 8;  // a tower's columns of cat / dcat
  auto alloc0 = [&](float **q, size_t bytes) -> bool { return t->own.alloc(q, bytes, true) == MPN_OK; };
  bool ok = alloc0(&t->cat, (size_t)T * Fcb * rec) && alloc0(&t->dcat, (size_t)T * Fcb * rec);
  size_t part = 0;
  for (int i = 0; i < T && ok; ++i) {
    const mpn_frcnn::Tower &W = p->towers[i];
    LinT mix{W.mix_w, W.mix_b, W.total_feat, c5, 1, 0}, fc6{W.w6, W.b6, p->K6, F, PP, 1}, fc7{W.w7, W.b7, F, F, 1, 1};
    ok = alloc0(&mix.x, (size_t)(round_up(mix.K, 64) / 8) * PP * rec) && alloc0(&mix.y, std::max((size_t)(lin_np(c5) / 8) * PP * rec, k6_rec)) &&
         alloc0(&fc6.y, (size_t)Fcb * rec) && alloc0(&mix.g, k6_rec) && alloc0(&fc6.g, (size_t)Fcb * rec);
    mix.nseg = PP;
    fc6.x = mix.y; fc6.dx = mix.g; fc6.masked = 0; fc6.drop = 2 * i;
    fc7.x = fc6.y; fc7.dx = fc6.g; fc7.y = t->cat + (size_t)i * slice; fc7.g = t->dcat + (size_t)i * slice; fc7.drop = 2 * i + 1;
    t->lin.insert(t->lin.end(), {mix, fc6, fc7});
    part = std::max(part, seg_wgrad_part_elems(mix.K, c5, PP));
  }
  LinT cls{p->wcls, p->bcls, nf * F, KC, 1, 0}, bbox{p->wbbox, p->bbbox, F, 4 * C, 1, 0};  // on the Foveal towers' concat; on the het tower
  cls.x = t->cat; cls.dx = t->dcat;
  bbox.x = t->cat + (size_t)nf * slice; bbox.dx = t->dcat + (size_t)nf * slice;
  ok = ok && alloc0(&cls.y_rm, M * KC * sizeof(float)) && alloc0(&bbox.y_rm, M * 4 * C * sizeof(float));
  ok = ok && alloc0(&cls.g, (size_t)(lin_np(KC) / 8) * rec) && alloc0(&bbox.g, (size_t)(lin_np(4 * C) / 8) * rec);
  t->lin.insert(t->lin.end(), {cls, bbox});
  for (LinT &L : t->lin) ok = ok && alloc_momentum(t->own, L);  // every layer is trained
  t->bwd = {3 * T, 3 * T + 1};
  for (int i = 0; i < T; ++i) t->bwd.insert(t->bwd.end(), {3 * i + 2, 3 * i + 1, 3 * i});
  ok = ok && alloc0(&t->seg_part, part * sizeof(float)) && alloc_core(p, *t);
  if (!t->kconv) return ok;
  // the conv block and what lies between it and the mix layers: per tower the gradient at its conv5 slab before and behind
  // nn.Normalize's backward, per distinct Foveal region conv5's raw pools and their argmax, the rows' windows, per image the map
  const size_t slab = (size_t)((c5 + 7) / 8) * PP * rec;
  for (int i = 0; i < T; ++i) if (std::find(t->regions.begin(), t->regions.end(), p->towers[i].region) == t->regions.end()) t->regions.push_back(p->towers[i].region);
  std::sort(t->regions.begin(), t->regions.end());
  t->gx.assign(T, nullptr); t->dx5.assign(T, nullptr);
  t->xraw.assign(t->regions.size(), nullptr); t->argmax.assign(t->regions.size(), nullptr);
  for (int i = 0; i < T && ok; ++i) {
    ok = alloc0(&t->gx[i], slab);
    if (p->conv345_norm) ok = ok && alloc0(&t->dx5[i], slab);
    else t->dx5[i] = t->gx[i];  // conv345_unnormalized: MulConstant(1) on the conv5 slab
  }
  for (size_t r = 0; r < t->regions.size() && ok; ++r)
    ok = alloc0(&t->xraw[r], slab) && t->own.alloc(&t->argmax[r], M * c5 * PP * sizeof(int32_t), true) == MPN_OK;
  ok = ok && alloc0(&t->pfov, M * 20 * sizeof(float));
  int mh = c.max_h, mw = c.max_w;
  final_map_size(p, &mh, &mw);
  t->g5_img = act_bytes(c5, mh, mw) / sizeof(float);
  ok = ok && alloc0(&t->g5, t->g5_img * MPN_TRAIN_MAX_IMAGES * sizeof(float));
  return ok && alloc_conv_block(p, t, t->own);
}

// mpn_mpnet_train_begin and mpn_mpnet_train_begin_conv behind their `p != nullptr` (fn: the entry point's name)
static int mpnet_train_begin(mpn_frcnn *p, const char *fn, int conv_layers, float momentum, float weight_decay, float bbox_weight) {
  int rc = begin_refusals(p, true, fn);
  if (rc) return rc;
  const int K = conv_layers_above_last_pool(p);
  if (conv_layers < 0 || conv_layers > K) {
    set_error("%s: invalid argument: conv_layers = %d, but k runs from 0 to K = %d on this trunk: the conv layers above its last pooling layer (a pooling layer has no backward pass here)",
              fn, conv_layers, K);
    return MPN_EINVAL;
  }
  std::unique_ptr<TowerTrainState> t(new TowerTrainState());
  if ((rc = begin_core(*t, fn, momentum, weight_decay, bbox_weight)) != MPN_OK) return rc;
  t->kconv = conv_layers; t->first = (int)p->conv.size() - conv_layers; t->dgrad_wino = false;
  if (!alloc_tower_train_state(p, t.get()) || hipDeviceSynchronize() != hipSuccess) {
    set_error("%s: allocating the momentum / activation / gradient buffers failed: %s", fn, hipGetErrorString(hipGetLastError()));
    return MPN_ENOMEM;
  }
  p->tower_train = t.release();  // all or nothing: published last
  return MPN_OK;
}

extern "C" int mpn_mpnet_train_begin(mpn_frcnn *p, float momentum, float weight_decay, float bbox_weight) {
  MPN_CHECK_ARG(p != nullptr);
  return mpnet_train_begin(p, __func__, 0, momentum, weight_decay, bbox_weight);
}
extern "C" int mpn_mpnet_train_begin_conv(mpn_frcnn *p, int conv_layers, float momentum, float weight_decay, float bbox_weight) {
  MPN_CHECK_ARG(p != nullptr);
  return mpnet_train_begin(p, __func__, conv_layers, momentum, weight_decay, bbox_weight);
}

extern "C" int mpn_mpnet_train_end(mpn_frcnn *p) {
  MPN_CHECK_ARG(p != nullptr);
  return train_end(p, true, __func__);
}

// The body of mpn_mpnet_train_add on device row pointers, everything checked
static int mpnet_add_rows(mpn_frcnn *p, TowerTrainState *t, const float *d_image, int H0, int W0, int H, int W, double sc, const float *d_rois,
                          const float *d_gt, const int *d_labels, int n, hipStream_t s) {
  const mpn_frcnn_config &c = p->cfg;
  int rc = MPN_OK;
  p->seg_shape[0][0] = -1;  // (as run_detect) the trunk's buffers, the ROI and Foveal tables are rewritten: the next head segment runs for real
  Act feat;
  rc = obtain_features(p, d_image, H0, W0, H, W, sc, &p->up, s, &feat);  // getImages' rescale + the frozen trunk, exactly as detect
  // the maps now belong to a training image: nothing a detect on cached features may pool from, and no range-max table goes with them
  p->up.invalidate(); p->mir.invalidate();
  p->vmax_built[0] = p->vmax_built[1] = p->vmax_built[2] = false;
  if (rc) return rc;
  rc = mpn_project_im_rois(d_rois, n, sc, p->rois, s);
  if (rc == MPN_OK) rc = mpn_foveal_forward(p->rois, n, p->fov, s);
  if (rc) return rc;
  // conv345Combine in detect's in-place form (run_mpnet_head without the scale fold), one stream: per tower the ROI max-pools of its maps
  // over its Foveal region side by side, each map's slab normalised per ROI — the same launches, so the same bits: the pooling from the
  // pixel-major range-max tables with the sum of squares fused in (roi_pool_c8 + l2norm_scale_c8 pool the same values but add the squares
  // in another order: the norm's last bit differs).  The tables are detect's buffers, rebuilt here for this image's maps and left marked
  // unbuilt.  This image's rows go behind the pending ones: a shifted base pointer with the buffer's row pitch
  const int PP = c.pooled_h * c.pooled_w, Mp = p->Mp;
  const Act maps[3] = {feat, p->tap_act[1], p->tap_act[2]};
  const float scales[3] = {c.spatial_scale, c.spatial_scale * 2.0f, c.spatial_scale * 4.0f};
  const float kConv345Factor[3] = {1.0f, (float)(1.0 / 30), (float)(1.0 / 200)};  // model_utils.lua:231-237 (run_mpnet_head's)
  bool used_any[3] = {true, false, false};
  for (const mpn_frcnn::Tower &T : p->towers) { used_any[1] = used_any[1] || T.use4; used_any[2] = used_any[2] || T.use3; }
  for (int m = 0; m < 3 && rc == MPN_OK; ++m) if (used_any[m]) rc = build_vmax_tables_pm(maps[m], p->vmax_tab[m], s);
  if (rc) return rc;
  for (size_t i = 0; i < p->towers.size(); ++i) {
    const mpn_frcnn::Tower &T = p->towers[i];
    const int used[3] = {1, T.use4, T.use3};
    int cb_off = 0;
    for (int m = 0; m < 3; ++m) {
      if (!used[m]) continue;
      float *dst = t->mix((int)i).x + ((size_t)cb_off * PP * Mp + t->pending) * 8;
      rc = roi_pool_pm_rmq(maps[m], p->vmax_tab[m], p->fov + 5 * T.region, n, c.pooled_h, c.pooled_w, scales[m], RoiRule{1.0f, 0, c.roi_bin_rule}, dst, s, 20, Mp,
                           p->conv345_norm ? 1 : 0, p->conv345_norm ? 1000.0f : kConv345Factor[m]);
      if (rc) return rc;
      cb_off += maps[m].Cb();
    }
  }
  if (t->kconv) {  // what the backward pass below the operand reads: per region conv5's raw pools (nn.Normalize's input) and their argmax —
    // roi_pool_c8, whose pooled values are the range-max tables' —, the rows' windows, the block's maps
    for (size_t r = 0; r < t->regions.size(); ++r) {
      rc = roi_pool_c8(feat, p->fov + 5 * t->regions[r], n, c.pooled_h, c.pooled_w, scales[0], RoiRule{1.0f, 0, c.roi_bin_rule}, t->xraw[r] + (size_t)t->pending * 8,
                       t->argmax[r] + (size_t)t->pending * p->feat_c * PP, s, 20, Mp);
      if (rc) return rc;
    }
    MPN_CHECK_HIP(hipMemcpyAsync(t->pfov + (size_t)t->pending * 20, p->fov, (size_t)n * 20 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if ((rc = save_conv_maps(p, t, feat, H, W, t->pending, n, s)) != MPN_OK) return rc;
  }
  return append_rows(*t, __func__, d_rois, d_gt, d_labels, n, s);
}

// The backward pass below the mix layers (mpn_mpnet_train_begin_conv, k > 0).  Per tower: the mix layer's input
// gradient on its conv5 columns — linear_dgrad_c8 with K = c5 (the packed weight's first c5 / 8 chunks are the conv5 slab's) in ONE
// launch over the (PP - 1) * Mp + B rows from the first segment's first row to the last segment's last: a row's result depends on that
// row alone, so the stale rows between two segments cost Mp / B of the work and touch nothing valid — and nn.Normalize's backward on
// the valid rows.  Per image, in train_add order: the five Foveal poolings' backward added tower after tower into one zeroed map
// (roi_pool_backward_add: one chain per cell), the ReLU mask of conv5's output, then conv_chain_backward.  No weight is touched.
static int tower_conv_backward(mpn_frcnn *p, TowerTrainState *t, int B, hipStream_t s) {
  const mpn_frcnn_config &c = p->cfg;
  const int PP = c.pooled_h * c.pooled_w, Mp = p->Mp, c5 = p->feat_c, T = (int)p->towers.size();
  int rc = MPN_OK;
  for (int i = 0; i < T && rc == MPN_OK; ++i) {
    const LinT &L = t->mix(i);
    rc = linear_dgrad_c8(L.g, PP * Mp, (PP - 1) * Mp + B, L.N, L.w, c5, nullptr, t->gx[i], PP * Mp, s);
    if (rc == MPN_OK && p->conv345_norm)
      rc = normalize_backward_c8(t->xraw[t->region_slot(p->towers[i].region)], L.x, t->gx[i], t->dx5[i], Mp, B, c5, PP, 1000.0f, s);
  }
  for (int i = 0; i < t->n_img && rc == MPN_OK; ++i) {
    const int h = t->img_h[i], w = t->img_w[i];
    Act G = make_act(t->g5 + (size_t)i * t->g5_img, c5, h, w);
    MPN_CHECK_HIP(hipMemsetAsync(G.p, 0, t->g5_img * sizeof(float), s));  // the chain's +0.0 and the halo (the input gradient's padding)
    for (float *gm : t->gmap) MPN_CHECK_HIP(hipMemsetAsync(gm, 0, t->gmap_bytes, s));
    for (int tw = 0; tw < T && rc == MPN_OK; ++tw) {
      RoiBwd a{};
      a.g = t->dx5[tw]; a.argmax = t->argmax[t->region_slot(p->towers[tw].region)]; a.rois = t->pfov + 5 * p->towers[tw].region;
      a.by_batch = 0; a.n0 = t->img_row0[i]; a.n1 = a.n0 + t->img_rows[i];
      a.B = 1; a.C = c5; a.H = h; a.W = w; a.PH = c.pooled_h; a.PW = c.pooled_w; a.windows = (c.pooled_h <= 32 && c.pooled_w <= 32) ? 1 : 0;
      a.g_n = 8; a.g_cb = (long)PP * Mp * 8; a.g_c = 1; a.g_bin = (long)Mp * 8;
      a.o_b = 0; a.o_cb = (long)G.plane(); a.o_c = 1; a.o_y = (long)G.Wp * 8; a.o_x = 8;
      a.scale = c.spatial_scale; a.rr = RoiRule{1.0f, 0, c.roi_bin_rule};
      a.out = G.p + ((size_t)G.Wp + 1) * 8;
      rc = roi_pool_backward_add(a, 20, s);
    }
    // the pooled values are conv5's post-ReLU values, but nn.Normalize sits between the pooling and the ReLU: the gradient at a pooled
    // zero is not zero until this mask
    if (rc == MPN_OK) rc = relu_mask_c8p(G, train_map(p, t, t->acts + (size_t)i * t->act_img, t->kconv, false, t->img_nh[i], t->img_nw[i]), s);
    if (rc == MPN_OK) rc = conv_chain_backward(p, t, i, G, 1, s);  // (cur = 1: the first input gradient goes to gmap[0])
  }
  return rc;
}

extern "C" int mpn_mpnet_train_step(mpn_frcnn *p, float lr, float *d_loss, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  TrainCore *core;
  long step;
  int rc = step_begin(p, true, __func__, lr, &core, &step);
  if (rc) return rc;
  TowerTrainState *t = static_cast<TowerTrainState *>(core);
  const int B = t->pending, Mp = p->Mp, n = (int)t->lin.size();
  ScratchScope scratch_scope(&p->scratch);
  hipStream_t s = as_stream(stream);
  rc = lin_forward(t->lin.data(), n, *t, B, Mp, step, s);  // one stream, tower after tower, then the two heads
  if (rc) return rc;
  rc = train_loss_split(t->cls().y_rm, t->bbox().y_rm, B, p->cfg.n_classes, p->n_integral, t->head_k, t->rois, t->gt, t->labels, loss_cfg(p, *t), t->cls().g,
                        t->bbox().g, Mp, d_loss ? d_loss : t->loss, s);
  if (rc == MPN_OK) rc = lin_dgrad(t->lin.data(), t->bwd.data(), n, *t, B, Mp, s);
  if (rc == MPN_OK && t->kconv) rc = tower_conv_backward(p, t, B, s);  // every input gradient of the step before any update
  if (rc == MPN_OK) rc = lin_update(t->lin.data(), t->bwd.data(), n, *t, B, Mp, lr, t->seg_part, s);
  rc = conv_block_update(p, t, *t, lr, rc, s);
  step_end(*t);
  return rc;
}

static int refuse_not_mpnet(const mpn_frcnn *p, const char *fn) {
  if (p->is_mpnet) return MPN_OK;
  set_error("%s: not an mpn_mpnet_create handle: a %s handle has no towers to unpack", fn, handle_kind_name(p));
  return MPN_ESTATE;
}

extern "C" int mpn_mpnet_get_tower_weights(mpn_frcnn *p, int tower, float *d_mix_w, float *d_mix_b, float *d_fc6_w, float *d_fc6_b, float *d_fc7_w,
                                           float *d_fc7_b, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  if (int rc = refuse_not_mpnet(p, "mpn_mpnet_get_tower_weights")) return rc;
  if (tower < 0 || tower >= (int)p->towers.size()) { set_error("mpn_mpnet_get_tower_weights: tower %d of %d", tower, (int)p->towers.size()); return MPN_EINVAL; }
  const mpn_frcnn::Tower &W = p->towers[tower];
  const int F = p->cfg.fc_dim, c5 = p->feat_c;
  hipStream_t s = as_stream(stream);
  int rc = unpack_linear_weights(W.mix_w, W.mix_b, W.total_feat, c5, 1, 0, c5, d_mix_w, d_mix_b, s);
  if (rc == MPN_OK) rc = unpack_linear_weights(W.w6, W.b6, p->K6, F, p->cfg.pooled_h * p->cfg.pooled_w, 0, F, d_fc6_w, d_fc6_b, s);
  if (rc == MPN_OK) rc = unpack_linear_weights(W.w7, W.b7, F, F, 1, 0, F, d_fc7_w, d_fc7_b, s);
  return rc;
}

extern "C" int mpn_mpnet_get_head_weights(mpn_frcnn *p, float *d_cls_w, float *d_cls_b, float *d_bbox_w, float *d_bbox_b, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  if (int rc = refuse_not_mpnet(p, "mpn_mpnet_get_head_weights")) return rc;
  const int F = p->cfg.fc_dim, C = p->cfg.n_classes, KC = p->n_integral * C, nf = (int)p->towers.size() - 1;
  hipStream_t s = as_stream(stream);
  int rc = unpack_linear_weights(p->wcls, p->bcls, nf * F, KC, 1, 0, KC, d_cls_w, d_cls_b, s);
  if (rc == MPN_OK) rc = unpack_linear_weights(p->wbbox, p->bbbox, F, 4 * C, 1, 0, 4 * C, d_bbox_w, d_bbox_b, s);
  return rc;
}

// ---- the optimiser state of a tower run (mpn_mpnet_train_get_state / _set_state / _get_head_state / _set_head_state; DESIGN.md
// section 13.13): a table row's momentum in the Torch layout of its weight, through the packers the weights themselves go through ----
static int get_lin_state(const LinT &L, float *d_v, float *d_vb, hipStream_t s) {
  return unpack_linear_weights(L.v, L.vb, L.K, L.N, L.inner, 0, L.N, d_v, d_vb, s);
}
static int set_lin_state(const LinT &L, const float *d_v, const float *d_vb, hipStream_t s) {
  return pack_linear_weights(d_v, d_vb, L.K, L.N, L.inner, L.v, L.vb, s);
}
// a tower-state entry point up to its own arguments: a MultiPathNet handle that can train and has begun; setter: no rows pending
static int tower_state_begin(mpn_frcnn *p, const char *fn, bool setter, TowerTrainState **t) {
  int rc = refuse_train(p, true, fn);
  TrainCore *c = nullptr;
  if (rc == MPN_OK) rc = need_core(p, true, fn, &c);
  if (rc) return rc;
  if (setter && c->pending > 0) { set_error("%s: %d rows are pending: take the step (mpn_mpnet_train_step) first", fn, c->pending); return MPN_ESTATE; }
  *t = static_cast<TowerTrainState *>(c);
  return MPN_OK;
}
static int check_tower_index(const mpn_frcnn *p, const char *fn, int tower) {
  const int T = (int)p->towers.size();
  if (tower >= 0 && tower < T) return MPN_OK;
  set_error("%s: invalid argument: tower %d is outside [0, T) of this handle's T = %d towers", fn, tower, T);
  return MPN_EINVAL;
}
// a setter's tensors: every one is part of the state
static int need_all_tensors(const char *fn, const float *const *q, const char *const *names, int n) {
  for (int i = 0; i < n; ++i)
    if (!q[i]) { set_error("%s: invalid argument: %s is NULL: every tensor of the call is part of the state", fn, names[i]); return MPN_EINVAL; }
  return MPN_OK;
}
static const char *const kTowerStateNames[6] = {"d_mix_v", "d_mix_vb", "d_fc6_v", "d_fc6_vb", "d_fc7_v", "d_fc7_vb"};
static const char *const kTowerHeadStateNames[4] = {"d_cls_v", "d_cls_vb", "d_bbox_v", "d_bbox_vb"};

extern "C" int mpn_mpnet_train_get_state(mpn_frcnn *p, int tower, float *d_mix_v, float *d_mix_vb, float *d_fc6_v, float *d_fc6_vb, float *d_fc7_v,
                                         float *d_fc7_vb, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  TowerTrainState *t;
  int rc = tower_state_begin(p, __func__, false, &t);
  if (rc == MPN_OK) rc = check_tower_index(p, __func__, tower);
  if (rc) return rc;
  float *const q[6] = {d_mix_v, d_mix_vb, d_fc6_v, d_fc6_vb, d_fc7_v, d_fc7_vb};
  hipStream_t s = as_stream(stream);
  for (int i = 0; i < 3 && rc == MPN_OK; ++i) rc = get_lin_state(t->lin[3 * tower + i], q[2 * i], q[2 * i + 1], s);
  return rc;
}

extern "C" int mpn_mpnet_train_set_state(mpn_frcnn *p, int tower, const float *d_mix_v, const float *d_mix_vb, const float *d_fc6_v,
                                         const float *d_fc6_vb, const float *d_fc7_v, const float *d_fc7_vb, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  TowerTrainState *t;
  int rc = tower_state_begin(p, __func__, true, &t);
  if (rc == MPN_OK) rc = check_tower_index(p, __func__, tower);
  const float *const q[6] = {d_mix_v, d_mix_vb, d_fc6_v, d_fc6_vb, d_fc7_v, d_fc7_vb};
  if (rc == MPN_OK) rc = need_all_tensors(__func__, q, kTowerStateNames, 6);
  if (rc) return rc;
  hipStream_t s = as_stream(stream);
  for (int i = 0; i < 3 && rc == MPN_OK; ++i) rc = set_lin_state(t->lin[3 * tower + i], q[2 * i], q[2 * i + 1], s);
  return rc;
}

extern "C" int mpn_mpnet_train_get_head_state(mpn_frcnn *p, float *d_cls_v, float *d_cls_vb, float *d_bbox_v, float *d_bbox_vb, long *h_step,
                                              void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  TowerTrainState *t;
  int rc = tower_state_begin(p, __func__, false, &t);
  if (rc) return rc;
  hipStream_t s = as_stream(stream);
  rc = get_lin_state(t->cls(), d_cls_v, d_cls_vb, s);
  if (rc == MPN_OK) rc = get_lin_state(t->bbox(), d_bbox_v, d_bbox_vb, s);
  if (rc == MPN_OK && h_step) *h_step = t->step;
  return rc;
}

extern "C" int mpn_mpnet_train_set_head_state(mpn_frcnn *p, const float *d_cls_v, const float *d_cls_vb, const float *d_bbox_v,
                                              const float *d_bbox_vb, long step, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  TowerTrainState *t;
  int rc = tower_state_begin(p, __func__, true, &t);
  const float *const q[4] = {d_cls_v, d_cls_vb, d_bbox_v, d_bbox_vb};
  if (rc == MPN_OK) rc = need_all_tensors(__func__, q, kTowerHeadStateNames, 4);
  if (rc) return rc;
  if (step < 0) { set_error("%s: invalid argument: step %ld is negative", __func__, step); return MPN_EINVAL; }
  hipStream_t s = as_stream(stream);
  rc = set_lin_state(t->cls(), d_cls_v, d_cls_vb, s);
  if (rc == MPN_OK) rc = set_lin_state(t->bbox(), d_bbox_v, d_bbox_vb, s);
  if (rc == MPN_OK) t->step = step;
  return rc;
}

// ---- the conv block of a tower run: the trunk's weights back in Torch layout, the trained layers' momentum (mpn_frcnn_get_trunk_weights'
// and mpn_frcnn_train_get_trunk_state / _set_trunk_state's rules on a MultiPathNet handle) ----
extern "C" int mpn_mpnet_get_trunk_weights(mpn_frcnn *p, int layer, float *d_w, float *d_b, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  if (int rc = refuse_not_mpnet(p, "mpn_mpnet_get_trunk_weights")) return rc;
  if (layer < 0 || layer >= (int)p->conv.size()) { set_error("mpn_mpnet_get_trunk_weights: layer %d of a %d-layer trunk", layer, (int)p->conv.size()); return MPN_EINVAL; }
  const ConvLayer &L = p->conv[layer];
  return unpack_conv_weights(L.wpk, L.bpk, L.Cin, L.Cout, d_w, d_b, as_stream(stream));
}

extern "C" int mpn_mpnet_train_get_trunk_state(mpn_frcnn *p, int layer, float *d_v, float *d_vb, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  TowerTrainState *t; ConvT *T;
  int rc = tower_state_begin(p, __func__, false, &t);
  if (rc == MPN_OK) rc = block_layer(t, __func__, layer, &T);
  if (rc) return rc;
  const ConvLayer &L = p->conv[layer];
  return unpack_conv_weights(T->v, T->vb, L.Cin, L.Cout, d_v, d_vb, as_stream(stream));
}

extern "C" int mpn_mpnet_train_set_trunk_state(mpn_frcnn *p, int layer, const float *d_v, const float *d_vb, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  TowerTrainState *t; ConvT *T;
  int rc = tower_state_begin(p, __func__, false, &t);
  if (rc == MPN_OK) rc = block_layer(t, __func__, layer, &T);
  if (rc) return rc;
  if (t->pending > 0) { set_error("%s: %d rows are pending: take the step (mpn_mpnet_train_step) first", __func__, t->pending); return MPN_ESTATE; }
  if (!d_v || !d_vb) { set_error("%s: %s is NULL: a trained layer's state is its weight and its bias momentum", __func__, d_v ? "d_vb" : "d_v"); return MPN_EINVAL; }
  const ConvLayer &L = p->conv[layer];
  return pack_conv_weights(d_v, d_vb, L.Cin, L.Cout, T->v, T->vb, as_stream(stream));
}

// ---- the learning-rate drop on the momentum (*_train_scale_momentum; train.lua:321-335 dfdx:mul(state.decay)) ----
// every trained row of a layer table: the weight's momentum and the bias's, whole packed buffers (one launch each)
static int scale_lin_momentum(const LinT *rows, int n, float factor, hipStream_t s) {
  int rc = MPN_OK;
  for (int i = 0; i < n && rc == MPN_OK; ++i) {
    const LinT &L = rows[i];
    if (!L.v) continue;
    rc = scale_momentum(L.v, lin_wpk_elems(round_up(L.K, 64), L.N), factor, s);
    if (rc == MPN_OK) rc = scale_momentum(L.vb, (size_t)lin_np(L.N), factor, s);
  }
  return rc;
}

static int train_scale_momentum(mpn_frcnn *p, bool mpnet, const char *fn, float factor, void *stream) {
  int rc = refuse_train(p, mpnet, fn);
  TrainCore *c = nullptr;
  if (rc == MPN_OK) rc = need_core(p, mpnet, fn, &c);
  if (rc) return rc;
  if (!(std::isfinite(factor) && factor >= 0.0f) || std::signbit(factor)) {  // (-0.0f too: it would turn a pad lane's +0.0 into -0.0)
    set_error("%s: invalid argument: factor %g is not a finite number >= 0 (-0.0 is not taken either)", fn, (double)factor);
    return MPN_EINVAL;
  }
  if (c->pending > 0) {
    set_error("%s: %d rows are pending: take the step (%s_train_step) first — the rate drops between epochs", fn, c->pending, kind_prefix(mpnet));
    return MPN_ESTATE;
  }
  if (factor == 1.0f) return MPN_OK;  // v * 1 is v: nothing to launch
  hipStream_t s = as_stream(stream);
  if (mpnet) {
    const TowerTrainState *t = p->tower_train;
    rc = scale_lin_momentum(t->lin.data(), (int)t->lin.size(), factor, s);
    return rc == MPN_OK ? scale_conv_momentum(p, t, factor, s) : rc;
  }
  const TrainState *t = p->train;
  rc = scale_lin_momentum(t->fc, 3, factor, s);
  return rc == MPN_OK ? scale_conv_momentum(p, t, factor, s) : rc;
}

extern "C" int mpn_frcnn_train_scale_momentum(mpn_frcnn *p, float factor, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  return train_scale_momentum(p, false, __func__, factor, stream);
}
extern "C" int mpn_mpnet_train_scale_momentum(mpn_frcnn *p, float factor, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  return train_scale_momentum(p, true, __func__, factor, stream);
}

// mpn_frcnn_debug_tensor's "tower_train_*" names, all of the last mpn_mpnet_train_step, row-major: "tower_train_x.<t>" the mix operand
// [rows, Kcat_t, PH, PW] (valid until the next mpn_mpnet_train_add), "tower_train_y6.<t>" fc6's output behind the dropout [rows, F],
// "tower_train_cat" [rows, T * F], "tower_train_cls" [rows, K * C], "tower_train_bbox" [rows, 4C], "tower_train_g_cls" [rows, K * C]
int mpn::tower_train_debug_tensor(mpn_frcnn *p, const char *name, const float **d_ptr, size_t *n_elems) {
  TowerTrainState *t = p->tower_train;
  if (!t || t->last_rows <= 0) { set_error("mpn_frcnn_debug_tensor: '%s' needs a mpn_mpnet_train_step", name); return MPN_ESTATE; }
  const mpn_frcnn_config &c = p->cfg;
  const int R = t->last_rows, F = c.fc_dim, C = c.n_classes, KC = p->n_integral * C, T = (int)p->towers.size(), PP = c.pooled_h * c.pooled_w, Mp = p->Mp;
  const char *tail = name + 12;
  int ti = -1, ii = -1, ji = -1;
  const bool is_x = sscanf(tail, "x.%d", &ti) == 1, is_y6 = !is_x && sscanf(tail, "y6.%d", &ti) == 1;
  // the conv block's tensors (mpn_mpnet_train_begin_conv, k > 0; valid until the next mpn_mpnet_train_add): "tower_train_argmax.<region>",
  // "tower_train_gx5.<t>" / "tower_train_dx5.<t>" [rows, c5, PH, PW], "tower_train_g5.<i>" [c5, h, w], "tower_train_act.<i>.<j>"
  const bool is_am = !strncmp(tail, "argmax.", 7), is_gx = !strncmp(tail, "gx5.", 4), is_dx = !strncmp(tail, "dx5.", 4), is_g5 = !strncmp(tail, "g5.", 3),
             is_act = !strncmp(tail, "act.", 4);
  if (is_am || is_gx || is_dx || is_g5 || is_act) {
    if (!t->kconv) { set_error("mpn_frcnn_debug_tensor: '%s' needs a mpn_mpnet_train_step after mpn_mpnet_train_begin_conv with conv_layers > 0", name); return MPN_ESTATE; }
    const int c5 = p->feat_c;
    size_t nt = 0;
    MPN_CHECK_HIP(hipDeviceSynchronize());
    int rc = MPN_OK;
    if (is_am) {
      if (sscanf(tail + 7, "%d", &ti) != 1 || t->region_slot(ti) >= (int)t->regions.size()) { set_error("mpn_frcnn_debug_tensor: '%s': no tower of this handle pools that Foveal region", name); return MPN_EINVAL; }
      nt = (size_t)R * c5 * PP;
      if (int rcd = grow_dbg(p, nt * sizeof(float))) return rcd;
      rc = int_to_float(t->argmax[t->region_slot(ti)], nt, p->dbg, nullptr);
    } else if (is_gx || is_dx) {
      if (sscanf(tail + 4, "%d", &ti) != 1 || ti < 0 || ti >= T) { set_error("mpn_frcnn_debug_tensor: '%s': the handle has towers 0..%d", name, T - 1); return MPN_EINVAL; }
      nt = (size_t)R * c5 * PP;
      if (int rcd = grow_dbg(p, nt * sizeof(float))) return rcd;
      rc = launch_unpack_pooled(is_gx ? t->gx[ti] : t->dx5[ti], R, c5, PP, Mp, p->dbg);
    } else {
      const int got = is_g5 ? sscanf(tail + 3, "%d", &ii) : sscanf(tail + 4, "%d.%d", &ii, &ji);
      if (got != (is_g5 ? 1 : 2) || ii < 0 || ii >= t->last_img || (is_act && (ji < 0 || ji > t->kconv))) {
        set_error("mpn_frcnn_debug_tensor: '%s': the last step had %d images and maps 0..%d", name, t->last_img, t->kconv);
        return MPN_EINVAL;
      }
      const Act a = is_g5 ? make_act(t->g5 + (size_t)ii * t->g5_img, c5, t->img_h[ii], t->img_w[ii])
                          : train_map(p, t, t->acts + (size_t)ii * t->act_img, ji, false, t->img_nh[ii], t->img_nw[ii]);
      nt = (size_t)a.C * a.H * a.W;
      if (int rcd = grow_dbg(p, nt * sizeof(float))) return rcd;
      rc = c8p_to_nchw(a, p->dbg, nullptr);
    }
    if (rc) return rc;
    MPN_CHECK_HIP(hipDeviceSynchronize());
    *d_ptr = p->dbg; *n_elems = nt;
    return MPN_OK;
  }
  if ((is_x || is_y6) && (ti < 0 || ti >= T)) { set_error("mpn_frcnn_debug_tensor: '%s': the handle has towers 0..%d", name, T - 1); return MPN_EINVAL; }
  size_t n = 0;
  if (is_x) n = (size_t)R * t->mix(ti).K * PP;
  else if (is_y6) n = (size_t)R * F;
  else if (!strcmp(tail, "cat")) n = (size_t)R * T * F;
  else if (!strcmp(tail, "cls") || !strcmp(tail, "g_cls")) n = (size_t)R * KC;
  else if (!strcmp(tail, "bbox")) n = (size_t)R * 4 * C;
  else { set_error("mpn_frcnn_debug_tensor: unknown tensor '%s'", name); return MPN_EINVAL; }
  MPN_CHECK_HIP(hipDeviceSynchronize());
  if (int rcd = grow_dbg(p, n * sizeof(float))) return rcd;
  int rc = MPN_OK;
  if (is_x) rc = launch_unpack_pooled(t->mix(ti).x, R, t->mix(ti).K, PP, Mp, p->dbg);
  else if (is_y6) rc = c8_rows_to_rowmajor(t->fc6(ti).y, Mp, R, F, p->dbg, nullptr);
  else if (!strcmp(tail, "cat")) rc = c8_rows_to_rowmajor(t->cat, Mp, R, T * F, p->dbg, nullptr);  // the towers' blocks back to back == one C8 matrix
  else if (!strcmp(tail, "g_cls")) rc = c8_rows_to_rowmajor(t->cls().g, Mp, R, KC, p->dbg, nullptr);
  else MPN_CHECK_HIP(hipMemcpy(p->dbg, !strcmp(tail, "cls") ? t->cls().y_rm : t->bbox().y_rm, n * sizeof(float), hipMemcpyDeviceToDevice));
  if (rc) return rc;
  MPN_CHECK_HIP(hipDeviceSynchronize());
  *d_ptr = p->dbg; *n_elems = n;
  return MPN_OK;
}

#ifdef MPN_DEBUG_HOOKS

// tools/bench_train.py (debug flavour only): fc6's fused weight-gradient + SGD kernel issued `iters` times BACK TO BACK on the operands the
// last mpn_frcnn_train_step left (depth MPN_TRAIN_FC6), with lr = momentum = wd = 0 — the weights keep their values, the momentum
// buffer ends as the plain gradient; the traffic is the real step's: w and v read and written once.
extern "C" int mpn_debug_bench_train_fc6(mpn_frcnn *p, int iters, float *ms_out) {
  MPN_CHECK_ARG(p && iters > 0 && ms_out);
  TrainState *t = p->train;
  if (!t || t->n_fc < 3 || t->last_rows <= 0) { set_error("mpn_debug_bench_train_fc6: needs a mpn_frcnn_train_step at depth MPN_TRAIN_FC6"); return MPN_ESTATE; }
  const LinT &L = t->fc[0];
  return time_back_to_back(iters, ms_out, [&] { return sgd_wgrad_c8(L.g, p->Mp, L.x, p->Mp, t->last_rows, L.N, L.K, L.inner, L.w, L.v, 0.f, 0.f, 0.f, nullptr); });
}

// tools/bench_train.py (debug flavour only): conv3x3_wgrad (the MFMA kernel + its segment reduce) of the LAST trained conv layer issued
// `iters` times back to back on image 0 of the last mpn_frcnn_train_step at depth >= MPN_TRAIN_CONV(1); the gradient map holds whatever
// that step left (the kernel's time does not depend on values).  Overwrites that layer's dW sum: take a step afterwards before reading it.
extern "C" int mpn_debug_bench_train_wgrad(mpn_frcnn *p, int iters, float *ms_out) {
  MPN_CHECK_ARG(p && iters > 0 && ms_out);
  TrainState *t = p->train;
  if (!t || !t->kconv || t->last_img <= 0) { set_error("mpn_debug_bench_train_wgrad: needs a mpn_frcnn_train_step at depth >= MPN_TRAIN_CONV(1)"); return MPN_ESTATE; }
  const int k = t->kconv;
  const ConvLayer &L = p->conv[t->first + k - 1];
  const Act X = train_in_map(p, t, t->acts, k, t->img_nh[0], t->img_nw[0]), G = make_act(t->gmap[0], L.Cout, X.H, X.W);
  return time_back_to_back(iters, ms_out, [&] { return conv3x3_wgrad(X, G, t->part, t->cl[k - 1].dw, 0, nullptr); });
}

// tools/bench_train.py (debug flavour only): maxpool2x2_backward_c8p in its fused form issued `iters` times back to back on the LARGEST
// pooled trained layer of the last mpn_frcnn_train_step at depth MPN_TRAIN_TRUNK(k), k > K (image 0's saved pre-pool map; dY and dX are
// the two gradient maps with whatever that step left: the kernel's time does not depend on values).  *layer_out: that layer's index.
extern "C" int mpn_debug_bench_train_poolbwd(mpn_frcnn *p, int iters, float *ms_out, int *layer_out) {
  MPN_CHECK_ARG(p && iters > 0 && ms_out);
  TrainState *t = p->train;
  int jb = 0;
  for (int j = 1; t && j <= t->kconv; ++j) if (p->conv[t->first + j - 1].pool && !jb) jb = j;  // the lowest pooled layer has the largest map
  if (!t || !jb || t->last_img <= 0) { set_error("mpn_debug_bench_train_poolbwd: needs a mpn_frcnn_train_step at a depth MPN_TRAIN_TRUNK(k) that crosses a pooling layer"); return MPN_ESTATE; }
  const Act Y = train_map(p, t, t->acts, jb, false, t->img_nh[0], t->img_nw[0]);
  const Act dY = make_act(t->gmap[0], Y.C, (Y.H + 1) / 2, (Y.W + 1) / 2), dX = make_act(t->gmap[1], Y.C, Y.H, Y.W);
  if (layer_out) *layer_out = t->first + jb - 1;
  return time_back_to_back(iters, ms_out, [&] { return maxpool2x2_backward_c8p(Y, dY, dX, 1, nullptr); });
}


#endif

// mpn_frcnn_debug_tensor's training tensors (pipeline.h): "train_pooled", "train_y6", "train_y7", "train_dx6", "train_act.<i>.<j>"
int mpn::train_debug_tensor(mpn_frcnn *p, const char *name, const float **d_ptr, size_t *n_elems, bool *known) {
  const TrainState *t = p->train;
  const int PP = p->cfg.pooled_h * p->cfg.pooled_w;
  const bool pooled = !strcmp(name, "train_pooled"), dx6 = !strcmp(name, "train_dx6");
  const int yi = !strcmp(name, "train_y6") ? 1 : (!strcmp(name, "train_y7") ? 2 : 0);
  *known = pooled || dx6 || yi || !strncmp(name, "train_act.", 10);
  if (!*known) return MPN_OK;
  size_t nt = 0;
  if (yi) {  // fc6's / fc7's output of the last mpn_frcnn_train_step as the layer above read it (behind the dropout), [rows, fc_dim]: valid until the next step
    if (!t || t->last_rows <= 0) { set_error("mpn_frcnn_debug_tensor: '%s' needs a mpn_frcnn_train_step", name); return MPN_ESTATE; }
    MPN_CHECK_HIP(hipDeviceSynchronize());
    nt = (size_t)t->last_rows * p->cfg.fc_dim;
    if (int rcd = grow_dbg(p, nt * sizeof(float))) return rcd;
    if (int rcy = c8_rows_to_rowmajor(t->fc[yi].x, p->Mp, t->last_rows, p->cfg.fc_dim, p->dbg, nullptr)) return rcy;
    MPN_CHECK_HIP(hipDeviceSynchronize());
    *d_ptr = p->dbg; *n_elems = nt;
    return MPN_OK;
  }
  if (pooled) {  // fc6's operand of the last mpn_frcnn_train_step, [rows, C, PH, PW]: rows at pitch Mp, valid until the next train_add
    if (!t || t->last_rows <= 0) { set_error("mpn_frcnn_debug_tensor: 'train_pooled' needs a mpn_frcnn_train_step"); return MPN_ESTATE; }
  } else if (!t || !t->kconv || t->last_rows <= 0) {  // the conv block's saved maps [C,h,w] / the gradient at the pooled features
    set_error("mpn_frcnn_debug_tensor: '%s' needs a mpn_frcnn_train_step at depth >= MPN_TRAIN_CONV(1)", name);
    return MPN_ESTATE;
  }
  MPN_CHECK_HIP(hipDeviceSynchronize());
  if (pooled || dx6) {
    nt = (size_t)t->last_rows * p->feat_c * PP;
    if (int rcd = grow_dbg(p, nt * sizeof(float))) return rcd;
    if (int rcl = launch_unpack_pooled(pooled ? t->fc[0].x : t->dx6, t->last_rows, p->feat_c, PP, p->Mp, p->dbg)) return rcl;
  } else {
    int i = -1, j = -1;
    if (sscanf(name + 10, "%d.%d", &i, &j) != 2 || i < 0 || i >= t->last_img || j < 0 || j > t->kconv) {
      set_error("mpn_frcnn_debug_tensor: '%s': the last step had %d images and maps 0..%d", name, t->last_img, t->kconv);
      return MPN_EINVAL;
    }
    const Act a = train_map(p, t, t->acts + (size_t)i * t->act_img, j, false, t->img_nh[i], t->img_nw[i]);
    nt = (size_t)a.C * a.H * a.W;
    if (int rcd = grow_dbg(p, nt * sizeof(float))) return rcd;
    if (int rcc = c8p_to_nchw(a, p->dbg, nullptr)) return rcc;
  }
  MPN_CHECK_HIP(hipDeviceSynchronize());
  *d_ptr = p->dbg; *n_elems = nt;
  return MPN_OK;
}
