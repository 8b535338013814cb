// graph_internal.h — what the translation units of the graph executor share (resnet.hip, graph_pool.hip, resnet_debug.hip): the C8I
// batch, the graph's structs, the launch-form ids and their debug recorders, the knobs read on both sides of a file boundary, the bf16
// rounding helpers every kernel family rounds through, and the few host functions that cross files.  No kernel is declared here: a
// kernel lives in the file of the one host function that launches it.  resnet.h is the public face towards pipeline.hip.
#pragma once
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/mpn.h"
#include "resnet.h"

namespace mpn {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct ActI {  // C8I batch of maps: element (b, c, y, x) at ((c/8) * pitch + (b*H + y)*W + x) * 8 + c%8
  float *p;
  int B, C, H, W;
  const float *planar = nullptr;  // the image only: the same transformed pixels as [3][H][W] planes (the im2col first layer reads these)
  int Cb() const { return (C + 7) / 8; }
  size_t rows() const { return (size_t)B * H * W; }
  size_t pitch() const { return (rows() + 127) / 128 * 128; }  // rows per channel-block plane (a C8 matrix of `rows` rows)
};
inline size_t c8i_elems(int B, int C, int H, int W) {  // allocation size: planes rounded up to the GEMM's 128-column tiles
  return (size_t)(round_up(C, 128) / 8) * (((size_t)B * H * W + 127) / 128 * 128) * 8;
}

typedef unsigned short bf16_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// fp32 -> bf16, round to nearest even: gfx950's own conversion (v_cvt_pk_bf16_f32, two values per instruction).  Every kernel of the
// graph executor rounds through these two helpers, so kernels that share a K order stay bit-identical to each other.  (The bit-arithmetic form
// — add 0x7fff + lsb, shift — costs 4-5 VALU instructions per value; at 128 accumulators per lane that was 10-20 % of a convolution
// launch: VALU work never overlaps the wave's MFMAs on this chip.)
typedef __bf16 hwbf16x2 __attribute__((ext_vector_type(2)));
typedef float cvtf32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {  // bits 0-15 = bf16(lo), bits 16-31 = bf16(hi)
  const cvtf32x2 v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, hwbf16x2));
}
__device__ __forceinline__ bf16_t f2bf(float f) { return (bf16_t)(pack_bf16x2(f, 0.0f) & 0xffffu); }
// The ReLU of every bf16 convolution epilogue, switched by a wave-uniform flag: one v_med3_f32 (v, 0, +inf), which maps NaN to 0 (as
// Torch's Threshold does; include/mpn.h).  Off, the value passes untouched: a med3 against -inf would turn NaN into -inf.
__device__ __forceinline__ float relu_bf(float v, bool on) { return on ? __builtin_amdgcn_fmed3f(v, 0.0f, __builtin_inff()) : v; }
__device__ __forceinline__ float bf2f(bf16_t h) { return __uint_as_float((unsigned)h << 16); }

struct RnConv {
  int Cin = 0, Cout = 0, K = 0, stride = 1, pad = 0;  // square form (ResNet); KH/KW/sh/sw/ph/pw below are what the kernels use
  int KH = 0, KW = 0, sh = 1, sw = 1, ph = 0, pw = 0;
  float *wpk = nullptr, *bpk = nullptr;
  float *lin_w = nullptr, *lin_b = nullptr;  // 1x1 / stride 1 with Cin % 64 == 0: also packed for the tuned GEMM (linear_c8)
  float *col_w = nullptr, *col_b = nullptr;  // Cin == 3 (fp32): packed for the GEMM over im2col rows, k = tap * 3 + c
  float *wino = nullptr;                     // graph trunks / ResNet heads (fp32), 3x3 / stride 1 / pad 1: Winograd-transformed weights (dense.h conv3x3_c8p)
  float *mos_in = nullptr, *mos_out = nullptr;  // ResNet heads: the mosaic images (shared by the head's eligible convolutions), laid out for
  int mos_h = 0, mos_w = 0, mos_mx = 0, mos_rows = 0, mos_cols = 0;  //   mos_rows x mos_cols px = max_rois maps of mos_h x mos_w, mos_mx per mosaic row
  bf16_t *wpk16 = nullptr;                   // bf16 graph: [tap][nch2][CoutP][8]
  int norelu_c0 = 0, norelu_c1 = 0;          // output channels [c0, c1) skip the ReLU (fused siblings with mixed activations; multiples of 8)
  float *ws = nullptr;                       // the graph's split-K workspace
  size_t ws_bytes = 0;
};
struct RnBlock {
  std::vector<RnConv> convs;
  bool has_sc = false;
  RnConv sc;
};
struct GTensor {
  int C = 0, H = 0, W = 0;
  float *buf = nullptr;
  float *c8p = nullptr;       // trunk tensors a Winograd convolution reads or writes: the same map in the C8P layout
  int p_h = 0, p_w = 0;       // the dims c8p's zero halo is laid out for (re-zeroed when the image size changes)
  int alias_of = -1, alias_c_off = 0;  // >= 0: this tensor is channels [alias_c_off, alias_c_off + C) of tensor alias_of (fused sibling convolutions)
};
struct GOp {
  int kind = 0, src = 0, dst = 0, dst_c_off = 0, kh = 1, kw = 1, sh = 1, sw = 1, ph = 0, pw = 0, relu = 0;
  int src_c_off = 0, cin = 0, ceil_mode = 0;   // the op reads channels [src_c_off, src_c_off + cin) of src
  float lrn_alpha = 0.f, lrn_beta = 0.f, lrn_k = 1.f;
  RnConv conv;
  float *pool_bias = nullptr;  // average pool only: bias (+ ReLU if relu) applied after the pool (commuted pool -> pointwise convolution)
  bool from_rois = false;      // head graphs: a max-pool of the ROI-pooled input itself -> computed from the feature map (roi_maxpool_c8i_bf16_sorted_kernel)
  float *fc_w = nullptr, *fc_b = nullptr;  // head graphs (fp32): a convolution over the WHOLE pooled map (AlexNet's fc6) packed for the tuned GEMM, K = (channel block, bin)
};
struct ResNetGraph {
  // op-list mode (graph_build): branching graphs; tensor 0 = image (trunk) / ROI-pooled map (head)
  bool is_graph = false;
  std::vector<GOp> g_trunk;
  std::vector<std::vector<GOp>> g_heads;  // one op list per tower (1 for plain inceptionv3.lua), all over the same head tensors
  std::vector<GTensor> t_trunk, t_head;
  int feat_tensor = 0, out_tensor = 0;
  RnConv conv1;
  std::vector<RnBlock> trunk;
  std::vector<std::vector<RnBlock>> heads;  // one layer4 copy per tower (1 for plain resnet.lua)
  int feat_c = 0, out_c = 0, pooled = 14, max_rois = 0;
  bool bf16 = false;             // activations / conv weights in bf16 (fp32 accumulate); the cls / bbox head GEMM stays fp32
  float *img = nullptr;          // C8I image
  float *img_planar = nullptr;   // fp32 graphs: the transformed image as [3][H][W] planes too (im2col first layer)
  float *tb[4] = {nullptr, nullptr, nullptr, nullptr};  // trunk activations (rotating)
  float *hb[4] = {nullptr, nullptr, nullptr, nullptr};  // per-ROI head activations (rotating)
  size_t tb_elems = 0, hb_elems = 0;
  float *feat = nullptr;         // points into tb[]: layer3 output of the last trunk run
  int feat_h = 0, feat_w = 0, last_h = -1, last_w = -1;
  float *fc_x = nullptr;         // (bin, roi)-row ROI-pooled matrix [Cb][PP][round_up(max_rois, 128)][8] for a GOp with fc_w
  bf16_t *feat_sorted = nullptr; // order-preserving int16 re-coding of the cached feature map (bf16 ROI pooling), rebuilt per trunk run
  size_t feat_sorted_elems = 0;
  bool feat_sorted_valid = false;
  bf16_t *feat_vmax = nullptr;   // vertical range-max levels 1 .. feat_vmax_levels of feat_sorted (the fused ROI max-pool reads two rows per column)
  size_t feat_vmax_elems = 0;    // elements per level
  int feat_vmax_levels = 0;
  bool feat_vmax_valid = false;
  float *splitk_ws = nullptr;    // fp32 partial slabs of split-K convolutions (bf16 graph; one stream at a time, like tb / hb)
  int roi_bins = 0;              // MPN_ROI_BINS_* (resnet_set_roi_bins)
  // second tower LANE (graphs with more than one head): a second set of per-ROI activation buffers, so that towers 1, 3 can run on a
  // second stream beside towers 0, 2, 4 (resnet_head_forward's `lane`; pipeline.hip run_detect).  Weights, the feature map and its sorted /
  // range-max images are shared (read-only while the towers run: resnet_heads_prepare builds them before the lanes fork).
  std::vector<GTensor> t_head2;
  float *hb2[4] = {nullptr, nullptr, nullptr, nullptr};
  bool has_lane2 = false;
  DeviceOwner own;  // of every device buffer above (mpn_internal.h)
};
constexpr size_t SPLITK_WS_BYTES = (size_t)96 << 20;

int rn_alloc(ResNetGraph *g, float **p, size_t bytes);   // resnet.hip
int rn_regrow(ResNetGraph *g, float **p, size_t bytes);

// ---- knobs read on both sides of a file boundary (MPN_KNOB_SHARED: the default is written once, here) ----
MPN_KNOB_SHARED(int, g_graph_fuse, 511);  // mpn_debug_set_graph_fuse: bit 0 = fuse sibling pointwise convolutions, bit 1 = commute average-pool -> pointwise convolution, bit 2 = max-pools of the ROI-pooled input computed from the feature map, bit 3 = fully-connected head layers (whole-map / 1x1-map convolutions) on the tuned GEMM, bit 4 = the image layer (Cin = 3) as a GEMM over im2col rows, bit 5 = trunk 3x3 / stride-1 convolutions on dense.hip's Winograd kernel, bit 6 = the fused ROI max-pool (bit 2) reads vertical range-max tables of the map, bit 7 = ResNet heads' 3x3 / stride-1 convolutions on the Winograd kernel (mosaic image of the per-ROI maps), bit 8 = the fully-connected operand pooled by dense.hip's pixel-major kernel; 0 = run the op list as given
MPN_KNOB_SHARED(int, g_roi_invariant, 1);  // mpn_debug_set_roi_invariant: 0 = per-ROI layers pick kernel / split by batch size as round 3 did (tests, timing)
#ifdef MPN_DEBUG_HOOKS
// mpn_debug_set_tower_knock (tools/tower_knockout.py; timing only, garbage results): the CEILING of a first per-ROI layer that never reads a
// materialised pooled tensor (VERDICT r5 task 1, step 1).  bit 0: the ROI pooling launch of the bf16 heads is skipped; bit 1: the convolutions
// that read the pooled tensor (Mixed_7a's fused 1x1 768 -> 384; layer4 block 1's conv1 and shortcut) run the B-direct kernel with every pixel
// load hitting ONE resident 1-KiB window (ABL bit 5: nothing can fetch its operand cheaper than from the CU's own cache).
inline int g_tower_knock = 0;
inline int g_knock_arm = 0;  // the next `g_knock_arm` rn_conv calls are first-layer convolutions (armed by the caller)
inline bool knock_first() { return g_knock_arm > 0 && (g_tower_knock & 2); }
#else
constexpr bool knock_first() { return false; }
#endif
// Which launch rn_conv's call took (mpn_debug_conv_last_form: tests/test_gpu_conv_numerics.py asserts it per case)
enum ConvForm : int {
  CF_KC1 = 1, CF_KC2 = 2, CF_KC3 = 3, CF_KC4 = 4, CF_PF = 5,  // fp32: conv2d_c8i_kernel<KC>, conv2d_c8i_pf_kernel
  CF_MOSAIC = 10, CF_IM2COL = 11, CF_GEMM_FC = 12,            // the Winograd mosaic, im2col + GEMM, the GEMM's split-K form on 1x1 maps
  CF_GEMM_DIRECT = 13, CF_GEMM_RI = 14,                       // the pointwise GEMM (direct / row-invariant)
  CF_BDIR = 20,                                               // bf16: conv2d_c8i_bf16_bdir_kernel
  CF_DMA_256x128 = 21, CF_DMA_128x256 = 22, CF_DMA_256x256 = 23,  // the LDS-DMA kernel, couts x pixels
  CF_B_KP1 = 26, CF_B_KP2 = 27,                               // conv2d_c8i_bf16_kernel<KP>
  CF_DMA_NCH8 = 28, CF_DMA_W8 = 29,                           // debug flavour: the LDS-DMA kernel with 64-channel stages / in the 8-wave shape
  CF_BDIR2_DS3 = 32, CF_BDIR2_DS4 = 33, CF_BDIR8 = 38, CF_BDPP = 39,  // debug flavour: bdir_ver 2 / 3 / 8 / 9
  CF_SPLIT = 0x100,                                           // or-ed in: split K (the generic fp32 / the 128 x 128 bf16 kernel + a finalize kernel)
};
#ifdef MPN_DEBUG_HOOKS
inline int g_dbg_conv_form = 0;
#define RN_FORM(v) (g_dbg_conv_form = (v))
#else
#define RN_FORM(v) ((void)0)
#endif
// Which pooling / LRN launch ran (mpn_debug_graph_op, mpn_debug_head_pool: tests/test_gpu_graph_pool_numerics.py asserts it per case).  An
// id's high nibble is its stage, so one head forward records the ROI pooling, the fused max-pool and the closing average side by side.
enum PoolKernel : int {
  PK_NONE = 0,                                                                                          // nothing ran (debug flavour: the knocked-out ROI pooling)
  PK_MAX_F32 = 1, PK_MAX_BF16 = 2, PK_AVG_F32 = 3, PK_AVG_BF16 = 4, PK_AVG_BF16_SMALL = 5, PK_LRN = 6,  // graph_run's pool / LRN block
  PK_ROI_F32 = 16, PK_ROI_ROWS4 = 17, PK_ROI_BF16 = 18, PK_ROI_SORTED = 19, PK_ROI_PM = 20,             // resnet_head_forward: ROI pooling
  PK_ROI_SORTED_EXP = 21,                                                                               //   (debug flavour: the sorted kernel's mpn_debug_set_pool_exp variants)
  PK_ROIMAX_SORTED = 32, PK_ROIMAX_SORTED_TABLES = 33,                                                  //   the fused max-pool (with range-max tables)
  PK_GAVG_F32 = 48, PK_GAVG_BF16 = 49, PK_GAVG_BF16_LDS = 50,                                           //   the closing average
};
#ifdef MPN_DEBUG_HOOKS
inline int g_dbg_pool_kernel[4] = {0, 0, 0, 0};
#define RN_POOL(v) (g_dbg_pool_kernel[(v) >> 4] = (v))
#else
#define RN_POOL(v) ((void)0)
#endif

// ---- functions that cross files ----
// resnet.hip: the convolution dispatcher (rn_conv picks a ConvForm and launches by it)
int rn_pack(ResNetGraph *g, RnConv &c, const float *d_w, const float *d_b);
int rn_conv(const RnConv &c, ActI in, float *out, const float *res, int relu, hipStream_t s, ActI *o, bool allow_gemm = true, bool per_roi = false);
int rn_block(const RnBlock &blk, ActI x, float *const bufs[4], hipStream_t s, ActI *out, bool per_roi = false);
// graph_pool.hip: every pooling site picks a PoolKernel, records it (RN_POOL) and launches by switching on it
bool fast_pool_ok(const ResNetGraph *g);      // the row-per-thread ROI pooling kernels are on and the map's channel blocks come in fours
bool roi_maxpool_fused(const ResNetGraph *g);  // a head's max-pools of its pooled input are computed from the feature map (GOp::from_rois)
int heads_prepare_impl(ResNetGraph *g, int head, hipStream_t s);
int rn_image_transform(ResNetGraph *g, const float *d_image, int H, int W, const int *swap, double scale, const double *mean, const double *std, int has_std,
                       hipStream_t s);
int rn_stem_maxpool(ResNetGraph *g, const ActI &y, int OH, int OW, hipStream_t s);  // ResNet's max-pool 3x3 / 2, pad 1, of conv1's output into tb[1]
int rn_c8i_to_c8p(const GTensor &t, hipStream_t s);  // a trunk tensor's C8I map into its C8P form / back
int rn_c8p_to_c8i(const GTensor &t, hipStream_t s);
int rn_pool_op(const ResNetGraph *g, const GOp &op, const GTensor &src, const ActI &in, const GTensor &dst, const ActI &od, char *outp, int B, hipStream_t s);
int rn_roi_pool(ResNetGraph *g, int head, std::vector<GTensor> &t_head, float *pool_dst, const float *d_rois, int roi_stride, int N, float spatial_scale,
                bool fc_gemm, bool fuse_mp, hipStream_t s);
int rn_global_avg(const ResNetGraph *g, const ActI &cur, int N, float *d_feat_c8, int Mp, hipStream_t s);
// resnet.hip: the op lists (the debug entries run single ops through them)
int graph_dims(const std::vector<GOp> &ops, std::vector<GTensor> &ts, int h0, int w0);
int graph_parse(ResNetGraph *g, int n_ops, const mpn_graph_op *ops_in, int n_t, const int *tc, std::vector<GOp> &out, std::vector<GTensor> &ts,
                bool head = false);
int graph_run(ResNetGraph *g, const std::vector<GOp> &ops, std::vector<GTensor> &ts, int B, hipStream_t s, bool skip_from_rois = false,
              bool fc_gemm = false);

// a head op that max-pools the ROI-pooled input itself (all of tensor 0's channels, square, floor mode): GOp::from_rois.  (A macro, shared with
// mpn_debug_head_pool: the expression expands in place, so graph_build compiles to the code it had.)
#define MPN_GOP_POOLS_ROIS(op, c0) \
  ((op).kind == 1 && (op).src == 0 && (op).src_c_off == 0 && (op).cin == (c0) && (op).kh == (op).kw && (op).sh == (op).sw && (op).ph == (op).pw && !(op).ceil_mode)

}  // namespace mpn
