// pipeline.h — the pipeline handle (struct mpn_frcnn) and the few functions that pipeline.hip (the per-image detect path) and
// train_driver.hip (the mpn_frcnn_train_* entry points) need from each other.  Private to these two translation units.
#pragma once
#include <map>
#include <tuple>
#include <utility>
#include <vector>

#include "dense.h"
#include "resnet.h"

using namespace mpn;  // (as both translation units do: the structs below name Act, DeviceOwner, ... as pipeline.hip always has)

struct TrainState;  // the training state of a handle: defined in train_driver.hip, private to it
struct TowerTrainState;  // ... of a MultiPathNet handle's towers (mpn_mpnet_train_*): likewise; a handle holds the one of its kind

struct ConvLayer {
  int Cin, Cout, pool;
  float *wpk = nullptr, *bpk = nullptr, *wino = nullptr;  // direct-conv and Winograd-transformed weights
  float *w36 = nullptr;     // first layer (<= 4 input channels, no pool): the K = 36 formulation's weights
  float *out = nullptr;     // C8P buffer for the conv output (max image size)
  float *pooled = nullptr;  // C8P buffer for the pooled output (when pool)
};

struct mpn_frcnn {
  mpn_frcnn_config cfg;
  std::vector<int> cout, pool_after;
  std::vector<ConvLayer> conv;
  float *img_c8p = nullptr;
  std::vector<std::pair<float *, size_t>> act_bufs;  // for re-zeroing when the image size changes
  int last_h = -1, last_w = -1;                       // the (canvas) geometry the halos are laid for
  int keep_prepool_from = -1;                         // >= 0: run_trunk also writes the pre-pool map (L.out) of the pooled layers from this one up (mpn_frcnn_train_add only)
  int feat_c = 0;
  // One cached final trunk map (VGG trunks): what a detect on cached features pools from.  run_trunk fills the record it is handed and no other.
  struct CachedMap {
    Act act = Act{};           // the map
    float *buf = nullptr;      // where the trunk writes it (nullptr: the last layer's own buffer)
    float *pm = nullptr;       // its pixel-major copy (roi_pool_pm) ...
    bool pm_valid = false;     // ... once the first pooling after a trunk run has built it
    int h = -1, w = -1;        // network-input size of the image it was computed from (-1: none cached)
    void invalidate() { act = Act{}; h = w = -1; pm_valid = false; }
  };
  CachedMap up, mir;           // of the upright image; of the mirrored one (plain Fast R-CNN handles under mpn_frcnn_set_augment: buf and pm exist)
  // head
  int K6 = 0, Mp = 0, n_head = 0;
  float *w6 = nullptr, *b6 = nullptr, *w7 = nullptr, *b7 = nullptr, *wh = nullptr, *bh = nullptr;
  float *rois = nullptr, *x6 = nullptr, *y6 = nullptr, *y7 = nullptr, *head = nullptr;
  float *scores = nullptr, *bbox = nullptr, *bbox_raw = nullptr;
  // NMS-stage buffers: two sets so that image i's NMS (side stream) overlaps image i+1's trunk
  float *scored_b[2] = {nullptr, nullptr}, *keep_b[2] = {nullptr, nullptr}, *thresh_b[2] = {nullptr, nullptr};
  float *voted_b[2] = {nullptr, nullptr}, *voted = nullptr;      // bbox-voted tables (opt.test_bbox_voting)
  float *it_scores = nullptr, *it_bbox = nullptr, *it_boxes = nullptr;  // iterative localisation: rows of both passes
  float *scaled = nullptr, *scale_tmp = nullptr;  // getImages' rescaled image (ImageDetect.lua:34-43), grown on demand
  size_t scaled_bytes = 0, scale_tmp_bytes = 0;
  int *counts_b[2] = {nullptr, nullptr}, *keep_idx_b[2] = {nullptr, nullptr}, *n_keep_b[2] = {nullptr, nullptr};
  float *scored = nullptr, *keep = nullptr, *thresh = nullptr;   // set of the most recent call
  int *counts = nullptr, *keep_idx = nullptr, *n_keep = nullptr;
  hipStream_t side = nullptr;           // side stream (default priority: see create) for the heads and the NMS / top-k tail of the pipelined forms
  // Deferred heads (pipelined forms of the plain Fast R-CNN head): cls / bbox GEMM + softmax + decode + select of image i run on `side`
  // too, under image i + 1's first trunk layers — they are 51 us of kernels that leave most of the GPU idle.  What they read is held per
  // buffer set: fc7's output (y7_b) and a copy of the caller's boxes (boxes_b); join_tail(b) orders their reuse two calls later.
  hipStream_t defer_stream = nullptr;   // non-null while run_detect is to hand the heads over to it
  bool was_deferred = false;            // the previous pipelined call handed its heads over
  int defer_set = 0;
  float *y7_b[2] = {nullptr, nullptr}, *boxes_b[2] = {nullptr, nullptr}, *y7_last = nullptr;  // y7_last: where the last head left fc7's output
  hipEvent_t ev_fc7 = nullptr;
  hipEvent_t ev_head[2] = {nullptr, nullptr}, ev_tail[2] = {nullptr, nullptr};
  bool tail_pending[2] = {false, false};
  unsigned long long seq = 0;
  float *dbg = nullptr;
  size_t dbg_bytes = 0;
  int last_n = 0, last_rows = 0;
  // ---- MultiPathNet head (models/multipathnet.lua:64-120); empty for plain Fast R-CNN
  struct Tower { int region, use4, use3, total_feat; float *mix_w, *mix_b, *w6, *b6, *w7, *b7; unsigned short *w6_s3 = nullptr, *w7_s3 = nullptr; };
  bool is_mpnet = false;
  std::vector<int> rn_region;   // ResNet towers: Foveal region per tower (empty = plain resnet.lua)
  ResNetGraph *rn = nullptr;  // ResNet Fast R-CNN (mpn_resnet_create): trunk + per-ROI layer4 replace the VGG convs / fc6 / fc7
  int tap3 = -1, tap4 = -1, n_integral = 1;
  bool conv345_norm = true;  // model_conv345_norm (model_utils.lua:209): false = the MulConstant(1, 1/30, 1/200) branch
  std::vector<Tower> towers;
  float *fov = nullptr, *tx = nullptr, *ty = nullptr, *tz6 = nullptr, *cat = nullptr, *cls_rm = nullptr, *bbox_rm = nullptr;
  float *wcls = nullptr, *bcls = nullptr, *wbbox = nullptr, *bbbox = nullptr;
  Act tap_act[3];  // [1], [2]: conv4, conv3 of the last trunk run ([0], conv5, is the upright record's map: up.act)
  float *vmax_tab[3] = {nullptr, nullptr, nullptr};  // vertical range-max tables of the three maps (MultiPathNet ROI pools)
  bool vmax_built[3] = {false, false, false};         // built for the current tap_act maps (per map: the pooling stream builds a map's tables where its first pooling is enqueued)
  bool vmax_pm = false;                               // ... in the pixel-major form
  float *mix_scale = nullptr;                         // [2 tower parities][3][Mp]: per-(map, ROI) nn.Normalize scales the mix GEMM applies
  // tower t + 1's skip pooling (L2 -> L1 bound, no matrix work) runs on its own stream under tower t's GEMMs (matrix-bound):
  float *tx2 = nullptr;                               // second pooled-operand buffer (towers alternate between tx and tx2)
  // round 6: two towers that pool the SAME Foveal region, one's maps a prefix of the other's (models/multipathnet.lua:74-113: the "het"
  // tower = region 2 with conv5 + conv4 + conv3, tower 2 = region 2 with conv5 + conv4), share ONE pooled operand: the wider one is pooled
  // once into tx3, the narrower tower's mix GEMM reads its K prefix (the per-map nn.Normalize scales are per (map, region, ROI): the same)
  float *tx3 = nullptr;
  int share_provider = -1, share_consumer = -1;       // tower indices (-1: no such pair)
  // The pooling stream IS the side stream (the NMS / top-k tail's) since the end of round 6: the tail of image i - 1 runs under image i's
  // trunk and is long over when image i's first pooling is enqueued behind it, and the handle needs one stream fewer.  With a stream of its own
  // the host-fed form drove five streams on ROCm's four hardware queues, and whichever stream shared a queue with the upload stream waited
  // behind the upload's completion marker: 0.2 ms per image (configs[2] host-fed 13.26-13.31 -> 13.07-13.13 ms, profiles/r06_hw_queues.txt).
  hipStream_t pool_stream = nullptr;   // alias of `side` (never destroyed on its own); nullptr = no overlapped pooling (plain Fast R-CNN handles)
  bool pool_on_side = false;
  hipEvent_t ev_pool_done[3] = {nullptr, nullptr, nullptr}, ev_mix_done[3] = {nullptr, nullptr, nullptr}, ev_pool_go = nullptr;
  unsigned short *w6_s3 = nullptr, *x6_s3 = nullptr;  // MPN_FC_SPLIT3: fc6's weights (packed once) and operand (per image) as three bf16 planes
  unsigned short *w7_s3 = nullptr, *y6_s3 = nullptr;  // ... and fc7's
  unsigned short *ty_s3[2] = {nullptr, nullptr}, *tz6_s3[2] = {nullptr, nullptr};  // MultiPathNet towers: the per-lane fc6 / fc7 operands as planes
  // two tower LANES (round 6): the towers of one image are independent until the concat (ModelParallelTable.lua:195-242 ran them on
  // different GPUs), so towers 1, 3 run on the handle's second tower stream with their own mix / fc6 buffers beside towers 0, 2, 4 on the
  // caller's stream: one lane's short-K mix GEMM (6.1 block rounds on 256 CUs, 40 stages per tile) and the prologue / epilogue of every
  // launch run under the other lane's fc6 / fc7 instead of leaving the matrix pipe idle.  Pure scheduling: bit-identical results.
  hipStream_t tower_stream = nullptr;
  hipEvent_t ev_lane_go = nullptr, ev_lane_done = nullptr;
  float *ty2 = nullptr, *tz6_2 = nullptr;
  DeviceOwner own;  // every device buffer, stream and event below that lives as long as the handle (mpn_internal.h)
  Scratch scratch;  // split-K slabs, NMS masks, ... of THIS handle (bound to the calling thread by ScratchScope in every entry point)
  int device = 0;   // the handle lives on the device that was current at creation
  // host-fed throughput form (mpn_frcnn_test_one_pipelined_host): three staging sets filled by the copy stream
  hipStream_t copy = nullptr;
  static constexpr int kStage = 3;
  float *stage_img[kStage] = {}, *stage_boxes[kStage] = {};
  size_t stage_bytes[kStage] = {};
  hipEvent_t ev_up[kStage] = {}, ev_consumed[kStage] = {};
  bool used_pending[kStage] = {};
  unsigned long long up_seq = 0;
  // proposal sharding (mpn_frcnn_test_one_sharded): this rank's row / class records and the gathered ones, grown on demand
  float *sh_buf[4] = {nullptr, nullptr, nullptr, nullptr};
  size_t sh_bytes[4] = {0, 0, 0, 0};
  // ---- captured launch graphs (round 4): the kernel chain of a SEGMENT of the per-image path — the head (transform .. decode, the
  // iterative-localisation passes) or the tail (per-class NMS, voting, top-k) — is captured once per (pointers, shape) with
  // hipStreamBeginCapture on the handle's capture stream and replayed with hipGraphLaunch on the caller's stream: one host call instead
  // of 30-60 launches.  A segment is replayed only when (a) the previous execution of that segment kind on this handle had the same
  // shape — the host-side state a real run leaves (cached-feature flags, sizes) is then exactly what it would be — (b) no library buffer
  // was replaced since the capture (alloc_generation), (c) profiling is off.  Everything between the segments (cross-stream events,
  // the select kernel, uploads) stays ordinary stream work, so the pipelined forms keep their overlap.
  struct GraphKey {
    int kind; const void *a, *b, *c, *d; int i0, i1, i2, i3;
    bool operator<(const GraphKey &o) const {
      return std::tie(kind, a, b, c, d, i0, i1, i2, i3) < std::tie(o.kind, o.a, o.b, o.c, o.d, o.i0, o.i1, o.i2, o.i3);
    }
  };
  struct GraphEntry { hipGraphExec_t exec = nullptr; unsigned long long gen = 0, last_use = 0; bool failed = false; int seen = 0; hipStream_t last_stream = nullptr; bool launched = false; };
  unsigned long long graph_clock = 0;
  std::map<GraphKey, GraphEntry> graphs;
  // the last few caller-pointer keys seen ONCE, per segment kind (a small ring: the pipelined forms alternate two output buffer sets, a host
  // may rotate a handful): such a key enters `graphs` only at its second sighting while still in the ring, so a host that hands in fresh
  // buffers every call never occupies the cache
  static constexpr int kUnseen = 8;
  GraphKey unseen[4][kUnseen] = {};
  bool unseen_valid[4][kUnseen] = {};
  int unseen_next[4] = {0, 0, 0, 0};
  int graphs_on = 0;                 // mpn_frcnn_set_graphs / MPN_GRAPHS (opt-in: see create_handle)
  hipStream_t cap_stream = nullptr;  // capture happens here (the caller's stream may be the legacy NULL stream, which cannot capture)
  int seg_shape[4][4] = {{-1, -1, -1, -1}, {-1, -1, -1, -1}, {-1, -1, -1, -1}, {-1, -1, -1, -1}};  // shape of the last execution per segment kind
  long graph_replays = 0, graph_captures = 0;
  // ---- multi-scale testing (mpn_frcnn_set_scales): the image pyramid of the plain Fast R-CNN head
  int n_scales = 0;                             // >= 2: a pyramid of scale_targets; otherwise the single scale cfg.scale_target
  double scale_targets[MPN_MAX_SCALES] = {};
  double create_scale_target = 0.0;             // cfg.scale_target at creation (set_scales(0) restores it)
  float *ms_feat = nullptr, *ms_pm = nullptr;   // per-level final maps (C8P, canvas geometry) and their pixel-major copies
  size_t ms_slot = 0, ms_pm_slot = 0;           // floats between levels (sized for the max_h x max_w canvas)
  int ms_cap = 0;                               // levels allocated
  double ms_scales[MPN_MAX_SCALES] = {};        // s_l of the cached maps
  int ms_src[MPN_MAX_SCALES] = {};              // the level whose map level l uses (an earlier level with the same scale, or l)
  int ms_h0 = -1, ms_w0 = -1;                   // original image size of the cached maps (-1: none)
  bool ms_pm_valid = false;                     // the pixel-major copies go with the cached maps
  // ---- horizontal-flip test-time augmentation (mpn_frcnn_set_augment)
  int augment = 0;
  float *aug_img = nullptr;                     // the mirrored ORIGINAL image (grown on demand: an image that getImages scales down may exceed max_h x max_w)
  size_t aug_img_bytes = 0;
  float *aug_boxes = nullptr, *aug_scores = nullptr, *aug_bbox = nullptr;  // flipped boxes [M,4]; the upright half's tables kept aside [M,C], [M,4C]
  // ---- training the head (mpn_frcnn_train_*): exists between train_begin and train_end
  struct TrainState *train = nullptr;  // (train_driver.hip)
  struct TowerTrainState *tower_train = nullptr;  // mpn_mpnet_train_* (DESIGN.md section 13.9): between mpn_mpnet_train_begin and _end
  // optional per-kernel-group timing with HIP events recorded on the launch stream
  bool prof = false;
  std::vector<hipEvent_t> ev_pool;
  std::vector<int> ev_tag;   // one tag per (begin,end) pair
  size_t ev_used = 0;
  double prof_ms[MPN_PROF_NTAGS] = {0};
  long prof_cnt[MPN_PROF_NTAGS] = {0};
};

namespace mpn {
// The fused head of a plain Fast R-CNN handle is one Linear of (K + 4) * C rows [cls_0 | .. | cls_{K-1} | bbox]: K = 1 for
// mpn_frcnn_create and the plain ResNet / op-list handles (5C, as ever), mpn_frcnn_create_integral's n_integral otherwise
inline int plain_head_width(const mpn_frcnn *p) { return (p->n_integral + 4) * p->cfg.n_classes; }
// a plain VGG handle that holds K > 1 integral classifiers (tower models keep theirs behind the towers: cls_rm)
inline bool plain_integral(const mpn_frcnn *p) { return !p->is_mpnet && !p->rn && p->n_integral > 1; }

// ---- what the training driver needs from the pipeline (pipeline.hip)
int obtain_features(mpn_frcnn *p, const float *d_image, int H0, int W0, int H, int W, double sc, mpn_frcnn::CachedMap *m, hipStream_t s, Act *feat);
double getimages_size(int H0, int W0, double target, double cap, int *H, int *W);
void final_map_size(const mpn_frcnn *p, int *h, int *w);
const char *handle_kind_name(const mpn_frcnn *p);
int grow_dbg(mpn_frcnn *p, size_t bytes);
int launch_unpack_pooled(const float *xc8, int N, int C, int PP, int Mp, float *out);  // unpack_pooled_kernel on the NULL stream

// ---- what the pipeline needs from the training driver (train_driver.hip)
void free_train_state(mpn_frcnn *p);
// mpn_frcnn_debug_tensor's "train_*" names.  *known = false: none of them (nothing done, the caller goes on to its own refusal)
int train_debug_tensor(mpn_frcnn *p, const char *name, const float **d_ptr, size_t *n_elems, bool *known);
// the "tower_train_*" names (mpn_mpnet_train_*'s state); an unknown one is refused there
int tower_train_debug_tensor(mpn_frcnn *p, const char *name, const float **d_ptr, size_t *n_elems);

#ifdef MPN_DEBUG_HOOKS
// the mpn_debug_bench_* hooks' clock: two warm-up calls, then `iters` calls back to back on the NULL stream between two events of its own
template <typename F>
int time_back_to_back(int iters, float *ms_out, F call) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = MPN_OK;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) rc = MPN_EHIP;
  for (int i = 0; i < 2 && rc == MPN_OK; ++i) rc = call();
  if (rc == MPN_OK && (hipDeviceSynchronize() != hipSuccess || hipEventRecord(e0, nullptr) != hipSuccess)) rc = MPN_EHIP;
  for (int i = 0; i < iters && rc == MPN_OK; ++i) rc = call();
  float ms = 0.f;
  if (rc == MPN_OK && (hipEventRecord(e1, nullptr) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess)) rc = MPN_EHIP;
  if (rc == MPN_EHIP) set_error("mpn_debug_bench: a HIP call failed: %s", hipGetErrorString(hipGetLastError()));
  *ms_out = ms / iters;
  for (hipEvent_t e : {e0, e1}) if (e) (void)hipEventDestroy(e);
  return rc;
}
#endif
}  // namespace mpn
