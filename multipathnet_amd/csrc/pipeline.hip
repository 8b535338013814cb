// pipeline.hip — the fused per-image path: Tester_FRCNN:testOne -> ImageDetect:detect ->
// model:forward (models/vgg.lua:23-31) -> per-class NMS -> keep_top_k, as ONE stream of kernels with
// no host synchronisation between the image upload and the final detections.
//
// Memory plan (sized for 288 GB HBM, nothing is re-used to save bytes): every layer output has its
// own C8P buffer whose halo is zeroed once; packed weights (fc6 alone 411 MB) stay resident; the
// ROI-pooled matrix, fc activations, scored boxes and NMS outputs are fixed-capacity buffers
// allocated at create time.  The reference's 500-ROI chunking (ImageDetect.lua:116-124) is not
// needed: all ROIs go through each GEMM at once (rows are independent, results identical), so the
// fc weights stream from HBM once per image instead of twice.
#include <cmath>
#include <cstdlib>
#include <iterator>
#include <algorithm>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "dense.h"
#include "resnet.h"
#include "pipeline.h"

namespace mpn {
int launch_bbox_decode(const float *d_boxes, const float *d_deltas, int N, int C, float *d_out, int clamp, float im_w,
                       float im_h, hipStream_t s);

// softmax over head[:, 0:C] (row stride ld) -> scores [M,C]; one wave per row
__global__ __launch_bounds__(256) void head_softmax_kernel(const float *__restrict__ head, int ld, int M, int C,
                                                           float *__restrict__ scores) {
  int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const float *r = head + (size_t)row * ld;
  float mx = -INFINITY;
  for (int c = lane; c < C; c += 64) mx = fmaxf(mx, r[c]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
  float sum = 0.f;
  for (int c = lane; c < C; c += 64) sum += expf(r[c] - mx);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
  for (int c = lane; c < C; c += 64) scores[(size_t)row * C + c] = expf(r[c] - mx) / sum;
}

// BBoxNorm (modules/BBoxNorm.lua:28-29) + convertFrom (utils.lua:229-247) + optional clamp
// (Tester_FRCNN.lua:75-78) on head[:, C:5C]; thread per (roi, class)
__global__ void head_decode_kernel(const float *__restrict__ head, int ld, int col0, int M, int C, const float *__restrict__ boxes,
                                   int has_norm, float m0, float m1, float m2, float m3, float s0, float s1, float s2,
                                   float s3, int clamp, float im_w, float im_h, float *__restrict__ raw, float *__restrict__ out) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)M * C) return;
  int i = (int)(t / C), c = (int)(t - (size_t)i * C);
  const float *d = head + (size_t)i * ld + col0 + 4 * c;
  float d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3];
  if (has_norm) {
    d0 = d0 * s0; d0 = d0 + m0;
    d1 = d1 * s1; d1 = d1 + m1;
    d2 = d2 * s2; d2 = d2 + m2;
    d3 = d3 * s3; d3 = d3 + m3;
  }
  if (raw) { float *r = raw + 4 * t; r[0] = d0; r[1] = d1; r[2] = d2; r[3] = d3; }
  const float *bx = boxes + 4 * (size_t)i;
  float x1 = bx[0], y1 = bx[1], x2 = bx[2], y2 = bx[3];
  float xc = (x1 + x2) * 0.5f, yc = (y1 + y2) * 0.5f;
  float w = x2 - x1, h = y2 - y1;
  float p0 = d0 * w, p1 = d1 * h;
  float xtc = xc + p0, ytc = yc + p1;
  float wt = expf(d2) * w, ht = expf(d3) * h;
  float hw = wt * 0.5f, hh = ht * 0.5f;
  float o0 = xtc - hw, o1 = ytc - hh, o2 = xtc + hw, o3 = ytc + hh;
  if (clamp) {  // Tester_FRCNN.lua:75-78 — the first detect() of testOne only
    o0 = o0 < 1.0f ? 1.0f : (o0 > im_w ? im_w : o0);
    o2 = o2 < 1.0f ? 1.0f : (o2 > im_w ? im_w : o2);
    o1 = o1 < 1.0f ? 1.0f : (o1 > im_h ? im_h : o1);
    o3 = o3 < 1.0f ? 1.0f : (o3 > im_h ? im_h : o3);
  }
  float *o = out + 4 * t;
  o[0] = o0; o[1] = o1; o[2] = o2; o[3] = o3;
}

// Horizontal-flip test-time augmentation, the merge (include/mpn.h mpn_frcnn_set_augment): one thread per (roi, class).
// sA / bA: the upright half's tables; s_io / b_io: the mirrored half's on entry, the merged ones on return.  The mirrored boxes are
// flipped back as utils.flipBoxes does ((-x) + W) + 1, then (a + b) * 0.5f, then head_decode_kernel's clamp; every step rounded on its own.
__global__ void augment_merge_kernel(const float *__restrict__ sA, const float *__restrict__ bA, float *__restrict__ s_io,
                                     float *__restrict__ b_io, int M, int C, int clamp, float im_w, float im_h) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)M * C) return;
  s_io[t] = __fmul_rn(__fadd_rn(sA[t], s_io[t]), 0.5f);
  const float *a = bA + 4 * t;
  float *b = b_io + 4 * t;
  const float b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
  const float f0 = __fadd_rn(__fadd_rn(-b2, im_w), 1.0f), f2 = __fadd_rn(__fadd_rn(-b0, im_w), 1.0f);
  float o0 = __fmul_rn(__fadd_rn(a[0], f0), 0.5f), o1 = __fmul_rn(__fadd_rn(a[1], b1), 0.5f);
  float o2 = __fmul_rn(__fadd_rn(a[2], f2), 0.5f), o3 = __fmul_rn(__fadd_rn(a[3], b3), 0.5f);
  if (clamp) {
    o0 = o0 < 1.0f ? 1.0f : (o0 > im_w ? im_w : o0);
    o2 = o2 < 1.0f ? 1.0f : (o2 > im_w ? im_w : o2);
    o1 = o1 < 1.0f ? 1.0f : (o1 > im_h ? im_h : o1);
    o3 = o3 < 1.0f ? 1.0f : (o3 > im_h ? im_h : o3);
  }
  b[0] = o0; b[1] = o1; b[2] = o2; b[3] = o3;
}

// integral eval head (model_utils.lua:296-313): K classifiers -> softmax each -> mean over K.
// logits: row i's K * C values at logits + i * ld (ld == K * C: the tower models' contiguous [M, K*C]; the plain K-head handle's fused
// head has the box columns behind them); one wave per row; sum over k in k order, then * (1/K) like nn.Mean.
__global__ __launch_bounds__(256) void integral_softmax_mean_kernel(const float *__restrict__ logits, int ld, int M, int K, int C,
                                                                    float *__restrict__ scores) {
  int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const float inv = 1.0f / (float)K;
  // per k: max and sum over all C columns (wave reductions), then accumulate this lane's columns
  float accv[4] = {0.f, 0.f, 0.f, 0.f};  // supports C <= 256
  for (int k = 0; k < K; ++k) {
    const float *r = logits + (size_t)row * ld + (size_t)k * C;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, r[c]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    float sum = 0.f;
    for (int c = lane; c < C; c += 64) sum += expf(r[c] - mx);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    int q = 0;
    for (int c = lane; c < C; c += 64, ++q) accv[q] += expf(r[c] - mx) / sum;
  }
  int q = 0;
  for (int c = lane; c < C; c += 64, ++q) scores[(size_t)row * C + c] = accv[q] * inv;
}

// The four score / box kernels' launches, in one place each: the pipeline stages below and (debug flavour) mpn_debug_head_post run the same geometry.
static int launch_head_softmax(const float *head, int ld, int M, int C, float *scores, hipStream_t s) {
  hipLaunchKernelGGL(head_softmax_kernel, dim3(cdiv(M, 4)), dim3(256), 0, s, head, ld, M, C, scores);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}
static int launch_integral_softmax_mean(const float *logits, int ld, int M, int K, int C, float *scores, hipStream_t s) {
  hipLaunchKernelGGL(integral_softmax_mean_kernel, dim3(cdiv(M, 4)), dim3(256), 0, s, logits, ld, M, K, C, scores);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}
// mean4 / std4: the BBoxNorm constants; std4[0] == 0 means the model has no BBoxNorm (the deltas are used as they are)
static int launch_head_decode(const float *head, int ld, int col0, int M, int C, const float *boxes, const float *mean4, const float *std4, int clamp,
                              float im_w, float im_h, float *raw, float *out, hipStream_t s) {
  const bool norm = std4[0] != 0.0f;
  hipLaunchKernelGGL(head_decode_kernel, dim3((unsigned)cdiv_sz((size_t)M * C, 256)), dim3(256), 0, s, head, ld, col0, M, C, boxes,
                     norm ? 1 : 0, mean4[0], mean4[1], mean4[2], mean4[3], std4[0], std4[1], std4[2], std4[3], clamp, im_w, im_h, raw, out);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}
static int launch_augment_merge(const float *sA, const float *bA, float *s_io, float *b_io, int M, int C, int clamp, float im_w, float im_h, hipStream_t s) {
  hipLaunchKernelGGL(augment_merge_kernel, dim3((unsigned)cdiv_sz((size_t)M * C, 256)), dim3(256), 0, s, sA, bA, s_io, b_io, M, C, clamp, im_w, im_h);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// pooled C8 matrix [cb*PP+bin][Mp][8] -> reference order [N, C*PP] (debug / parity only)
__global__ void unpack_pooled_kernel(const float *__restrict__ xc8, int N, int C, int PP, int Mp, float *__restrict__ out) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)N * C * PP;
  if (t >= total) return;
  int bin = (int)(t % PP); size_t r = t / PP;
  int c = (int)(r % C); int n = (int)(r / C);
  out[t] = xc8[(((size_t)(c >> 3) * PP + bin) * Mp + n) * 8 + (c & 7)];
}

int launch_unpack_pooled(const float *xc8, int N, int C, int PP, int Mp, float *out) {
  hipLaunchKernelGGL(unpack_pooled_kernel, dim3((unsigned)cdiv_sz((size_t)N * C * PP, 256)), dim3(256), 0, nullptr, xc8, N, C, PP, Mp, out);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

__global__ void copy_cols_kernel(const float *__restrict__ src, int ld, int col0, int M, int ncols, float *__restrict__ dst) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)M * ncols) return;
  int m = (int)(t / ncols), c = (int)(t - (size_t)m * ncols);
  dst[t] = src[(size_t)m * ld + col0 + c];
}
// ---- proposal (ROI) sharding of one image (mpn_frcnn_shard_*): record pack / unpack ------------------------------------------
// Balanced contiguous partition of n items over `world` ranks: the first n % world ranks own one item more.
__host__ __device__ inline void shard_bounds(int n, int world, int rank, int *lo, int *hi) {
  const int base = n / world, rem = n % world;
  *lo = rank * base + (rank < rem ? rank : rem);
  *hi = *lo + base + (rank < rem ? 1 : 0);
}
__device__ inline void shard_owner(int item, int n, int world, int *rank, int *local) {
  const int base = n / world, rem = n % world, cut = rem * (base + 1);
  if (item < cut) { *rank = item / (base + 1); *local = item - *rank * (base + 1); }
  else { const int q = (item - cut) / base; *rank = rem + q; *local = item - cut - q * base; }
}

// this rank's joined score / box tables (P passes x n_local rows, pass-major) -> its row record
// [scores: P x chunk x C][boxes: P x chunk x 4C], rows at / beyond n_local zeroed
__global__ void shard_pack_rows_kernel(const float *__restrict__ sc, const float *__restrict__ bb, int n_local, int P, int C, int chunk,
                                       float *__restrict__ rec) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t ns = (size_t)P * chunk * C, nb = ns * 4;
  if (t >= ns + nb) return;
  const bool is_box = t >= ns;
  const size_t u = is_box ? t - ns : t;
  const int w = is_box ? 4 * C : C;
  const int col = (int)(u % w);
  const size_t r = u / w;
  const int i = (int)(r % chunk), k = (int)(r / chunk);
  float v = 0.0f;
  if (i < n_local) v = (is_box ? bb : sc)[((size_t)k * n_local + i) * w + col];
  rec[t] = v;
}

// all ranks' row records [world][rec_floats] -> the image's joined tables sc [P*N, C], bb [P*N, 4C] in the unsharded row order
__global__ void shard_unpack_rows_kernel(const float *__restrict__ all, int N, int world, int P, int C, int chunk, size_t rec_floats,
                                         float *__restrict__ sc, float *__restrict__ bb) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t ns = (size_t)P * N * C, nb = ns * 4;
  if (t >= ns + nb) return;
  const bool is_box = t >= ns;
  const size_t u = is_box ? t - ns : t;
  const int w = is_box ? 4 * C : C;
  const int col = (int)(u % w);
  const size_t r = u / w;
  const int row = (int)(r % N), k = (int)(r / N);
  int owner, i;
  shard_owner(row, N, world, &owner, &i);
  const size_t plane = is_box ? (size_t)P * chunk * C : 0;
  (is_box ? bb : sc)[u] = all[(size_t)owner * rec_floats + plane + ((size_t)k * chunk + i) * w + col];
}

// class record of one rank: [n_keep: cmax ints][keep: cmax x rows x 5][keep_idx: cmax x rows ints][voted: cmax x rows x 5 (if voting)]
__host__ __device__ inline size_t shard_class_rec_floats(int cmax, int rows, int voting) {
  return (size_t)cmax * (1 + (size_t)rows * (voting ? 11 : 6));
}
// grid (ceil(rows / 256), cmax): slot j = class c0 + j of this rank's range [c0, c1)
__global__ void shard_pack_classes_kernel(const float *__restrict__ keep, const int *__restrict__ kidx, const int *__restrict__ n_keep,
                                          const float *__restrict__ voted, int c0, int c1, int rows, int cmax, float *__restrict__ rec) {
  const int j = blockIdx.y, c = c0 + j, i = blockIdx.x * blockDim.x + threadIdx.x;
  int *rn = reinterpret_cast<int *>(rec);
  const int n = c < c1 ? min(max(n_keep[c], 0), rows) : 0;
  if (i == 0) rn[j] = n;
  if (i >= n) return;
  float *rk = rec + cmax + ((size_t)j * rows + i) * 5;
  const float *k = keep + ((size_t)c * rows + i) * 5;
  rk[0] = k[0]; rk[1] = k[1]; rk[2] = k[2]; rk[3] = k[3]; rk[4] = k[4];
  reinterpret_cast<int *>(rec + cmax + (size_t)cmax * rows * 5)[(size_t)j * rows + i] = kidx[(size_t)c * rows + i];
  if (voted) {
    float *rv = rec + cmax + (size_t)cmax * rows * 6 + ((size_t)j * rows + i) * 5;
    const float *v = voted + ((size_t)c * rows + i) * 5;
    rv[0] = v[0]; rv[1] = v[1]; rv[2] = v[2]; rv[3] = v[3]; rv[4] = v[4];
  }
}
// all ranks' class records -> the image's per-class tables; grid (ceil(rows / 256), n_cls)
__global__ void shard_unpack_classes_kernel(const float *__restrict__ all, int n_cls, int world, int rows, int cmax, size_t rec_floats,
                                            float *__restrict__ keep, int *__restrict__ kidx, int *__restrict__ n_keep,
                                            float *__restrict__ voted) {
  const int c = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  int owner, j;
  shard_owner(c, n_cls, world, &owner, &j);
  const float *rec = all + (size_t)owner * rec_floats;
  const int n = min(max(reinterpret_cast<const int *>(rec)[j], 0), rows);
  if (i == 0) n_keep[c] = n;
  if (i >= n) return;
  const float *rk = rec + cmax + ((size_t)j * rows + i) * 5;
  float *k = keep + ((size_t)c * rows + i) * 5;
  k[0] = rk[0]; k[1] = rk[1]; k[2] = rk[2]; k[3] = rk[3]; k[4] = rk[4];
  kidx[(size_t)c * rows + i] = reinterpret_cast<const int *>(rec + cmax + (size_t)cmax * rows * 5)[(size_t)j * rows + i];
  if (voted) {
    const float *rv = rec + cmax + (size_t)cmax * rows * 6 + ((size_t)j * rows + i) * 5;
    float *v = voted + ((size_t)c * rows + i) * 5;
    v[0] = rv[0]; v[1] = rv[1]; v[2] = rv[2]; v[3] = rv[3]; v[4] = rv[4];
  }
}
}  // namespace mpn

using namespace mpn;

struct ProfScope {
  mpn_frcnn *p; hipStream_t s; bool on;
  ProfScope(mpn_frcnn *p_, int tag, hipStream_t s_) : p(p_), s(s_), on(p_->prof) {
    if (!on) return;
    if (p->ev_used + 2 > p->ev_pool.size()) {
      for (int i = 0; i < 64; ++i) { hipEvent_t e; if (p->own.event(&e, true) != MPN_OK) { on = false; return; } p->ev_pool.push_back(e); }
    }
    p->ev_tag.push_back(tag);
    (void)hipEventRecord(p->ev_pool[p->ev_used], s);
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(p->ev_pool[p->ev_used + 1], s);
    p->ev_used += 2;
  }
};

MPN_KNOB(int, g_fuse_pool, 1);
MPN_KNOB(int, g_first_k36, 1);  // 0: the first layer on the generic direct kernel
MPN_KNOB(int, g_roi_pool_pm, 1);  // 0: ROI pooling straight from the C8P map (roi_pool_c8_kernel)
MPN_KNOB(int, g_mix_fold, 1);     // 0: MultiPathNet's nn.Normalize scales applied in place (l2norm_apply) instead of inside the mix GEMM
MPN_KNOB(int, g_tower_lanes, 1);  // 0: the towers of an image one after the other on the caller's stream (rounds 2-5) instead of two lanes (mpn_debug_set_tower_lanes)
#ifdef MPN_DEBUG_HOOKS
static int g_mpn_pool_knock = 0;
extern "C" void mpn_debug_set_mpn_pool_knock(int v) { g_mpn_pool_knock = v; }
#endif
MPN_KNOB(int, g_mix_packed, 1);   // 0: the mix GEMM's rows padded to 128 per bin as the fc operands are (rounds 2-5; mpn_debug_set_mix_packed)
MPN_KNOB(int, g_tables_lazy, 1);  // 0: all range-max tables on the launch stream in front of the head (rounds 3-5) instead of per map on the pooling stream (mpn_debug_set_tables_lazy)
MPN_KNOB(int, g_tower_order, 1);  // 0: the towers in index order instead of cheapest pooling first (mpn_debug_set_tower_order)
MPN_KNOB(int, g_tower_share, 1);  // 0: every tower pools its own operand even where two of them pool the same region's maps (mpn_debug_set_tower_share)
MPN_KNOB(int, g_pool_overlap, 1); // 0: MultiPathNet's skip pooling on the launch stream instead of its own stream under the previous tower's GEMMs
MPN_KNOB(int, g_defer_heads, 1);  // 0: the pipelined forms keep heads / softmax / decode / select on the launch stream (rounds 1-5a); 2 (test): the
                                  // side stream is held back 1 ms before the heads, so that the launch stream runs far ahead of it
#ifdef MPN_DEBUG_HOOKS
__global__ void side_stream_delay_kernel(long long ticks) {  // wall_clock64: 100 MHz
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}
#endif
MPN_KNOB(int, g_halo_memset, 0);  // 1: a size change clears every activation buffer whole (rounds 1-4) instead of re-laying the halos only
#ifdef MPN_DEBUG_HOOKS
extern "C" void mpn_debug_set_fuse_pool(int v) { g_fuse_pool = v; }
extern "C" void mpn_debug_set_first_k36(int v) { g_first_k36 = v; }
extern "C" void mpn_debug_set_roi_pool_pm(int v) { g_roi_pool_pm = v; }
extern "C" void mpn_debug_set_mix_fold(int v) { g_mix_fold = v; }
extern "C" void mpn_debug_set_pool_overlap(int v) { g_pool_overlap = v; }
extern "C" void mpn_debug_set_tower_lanes(int v) { g_tower_lanes = v; }
extern "C" void mpn_debug_set_tower_share(int v) { g_tower_share = v; }
extern "C" void mpn_debug_set_tower_order(int v) { g_tower_order = v; }
extern "C" void mpn_debug_set_tables_lazy(int v) { g_tables_lazy = v; }
extern "C" void mpn_debug_set_mix_packed(int v) { g_mix_packed = v; }
extern "C" void mpn_debug_set_halo_memset(int v) { g_halo_memset = v; }
extern "C" void mpn_debug_set_defer_heads(int v) { g_defer_heads = v; }
#endif

// the final trunk map's size for an h x w network input: halved (rounding up) at every pooling layer
void mpn::final_map_size(const mpn_frcnn *p, int *h, int *w) {
  for (auto &L : p->conv) if (L.pool) { *h = (*h + 1) / 2; *w = (*w + 1) / 2; }
}
// getImages (ImageDetect.lua:34-43): s = target / min side, capped so that round(s * max side) <= cap (cap <= 0: none); the image is
// resampled to (long)(H0 * s) x (long)(W0 * s), or kept as it is when s == 1.  Returns s.
double mpn::getimages_size(int H0, int W0, double target, double cap, int *H, int *W) {
  const double sc = mpn_pick_scale(H0, W0, target, cap > 0.0 ? cap : 1e30);
  *H = H0; *W = W0;
  if (sc != 1.0) { *H = (int)((double)H0 * sc); *W = (int)((double)W0 * sc); }
  return sc;
}
// localisation passes whose rows reach the NMS (Tester_FRCNN.lua:91-100: use_rbox_scores drops one)
static int n_passes(const mpn_frcnn_config &c) { return c.num_iter > 1 ? (c.use_rbox_scores ? c.num_iter - 1 : c.num_iter) : 1; }
// the score / box tables the tail reads: the joined rows of all passes (utils.joinTable, Tester_FRCNN.lua:99-100), or the single pass's
static void joined_tables(const mpn_frcnn *p, float **scores, float **bbox) {
  const bool joined = p->cfg.num_iter > 1;
  *scores = joined ? p->it_scores : p->scores; *bbox = joined ? p->it_bbox : p->bbox;
}
const char *mpn::handle_kind_name(const mpn_frcnn *p) {
  return p->is_mpnet ? "MultiPathNet (mpn_mpnet_create)" : "ResNet / op-list (mpn_resnet_create / mpn_graph_create)";
}

// Everything the handle holds on the device goes back through its DeviceOwner (mpn_internal.h): no buffer, stream or event is named here.
extern "C" void mpn_frcnn_destroy(mpn_frcnn *p) {
  if (!p) return;
  (void)hipDeviceSynchronize();
  for (auto &kv : p->graphs) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
  p->own.release_streams();
  p->scratch.release();
  p->own.release_buffers();
  resnet_free(p->rn);
  free_train_state(p);
  delete p;
}

// ---- create: config checks, then one builder per part of the handle.  The builders allocate in a fixed order (trunk, graph net, towers /
// classifier or plain head, tail): placement in HBM is part of what the headline was measured with.
#define TRY(x) do { const int rc_ = (x); if (rc_ != MPN_OK) return rc_; } while (0)

struct CreateArgs {
  const mpn_frcnn_config *cfg;
  const float *const *conv_w, *const *conv_b;
  const float *fc6_w, *fc6_b, *fc7_w, *fc7_b, *cls_w, *cls_b, *bbox_w, *bbox_b;
  const mpn_mpnet_weights *mw; const mpn_resnet_weights *rw; const mpn_graph_weights *gw;  // at most one of them
  int n_integral = 1;  // none of them (mpn_frcnn_create_integral): the K classifiers stacked in cls_w / cls_b
  bool graph_net() const { return rw || gw; }  // the trunk / per-ROI stage live in a ResNetGraph object
  int tower_heads() const { return rw ? rw->n_heads : (gw ? gw->n_heads : 0); }  // > 1: MultiPathNet towers on a ResNet / op-list backbone
};

// packed weights and bias of one linear layer [N, K] (`inner`: see pack_linear_weights)
static int pack_linear(mpn_frcnn *p, const float *w, const float *b, int K, int N, int inner, float **wpk, float **bpk) {
  TRY(p->own.alloc(wpk, lin_wpk_elems(round_up(K, 64), N) * sizeof(float)));
  TRY(p->own.alloc(bpk, (size_t)lin_np(N) * sizeof(float)));
  return pack_linear_weights(w, b, K, N, inner, *wpk, *bpk, nullptr);
}
// MPN_FC_SPLIT3: the packed fp32 weights [K/8][NP][8] split once into three bf16 planes [3][K/8][NP↑256][8] (include/mpn.h)
static int pack_split3(mpn_frcnn *p, const float *wpk, int K, int N, unsigned short **planes) {
  TRY(p->own.alloc(planes, split3_plane_elems(K, lin_np(N)) * sizeof(unsigned short), true));
  return split3_planes(wpk, K, lin_np(N), lin_np(N), *planes, nullptr);
}

// Everything that can be refused from the descriptors alone, before a handle or a byte of device memory exists.
static int check_config(const CreateArgs &a) {
  const mpn_frcnn_config *cfg = a.cfg;
  MPN_CHECK_ARG(cfg && a.cls_w && a.bbox_w);
  const bool graph_net = a.graph_net();
  MPN_CHECK_ARG(graph_net || (a.conv_w && a.conv_b));
  MPN_CHECK_ARG(graph_net || a.mw || (a.fc6_w && a.fc7_w));
  MPN_CHECK_ARG(graph_net || (cfg->n_conv > 0 && cfg->conv_cout && cfg->pool_after && cfg->fc_dim > 0));
  MPN_CHECK_ARG(cfg->pooled_h > 0 && cfg->pooled_w > 0 && cfg->n_classes > 1);
  MPN_CHECK_ARG(cfg->max_h > 0 && cfg->max_w > 0 && cfg->max_rois > 0 && cfg->max_rois <= MPN_NMS_MAX_BOXES);
  MPN_CHECK_ARG(cfg->top_k > 0);
  // the image transforms (dense.h image_transform_c8p, the graph's rn_image_transform) index the image's three planes by tf_swap unchecked
  for (int j = 0; j < 3; ++j) MPN_CHECK_ARG(cfg->tf_swap[j] >= 0 && cfg->tf_swap[j] < 3);
  if (!(cfg->fc_arith == MPN_FC_FP32 || (cfg->fc_arith == MPN_FC_SPLIT3 && !graph_net))) { set_error("mpn_frcnn_config.fc_arith: %d (MPN_FC_SPLIT3 is for mpn_frcnn_create / mpn_mpnet_create pipelines)", cfg->fc_arith); return MPN_EINVAL; }
  if (cfg->roi_bin_rule != MPN_ROI_BINS_CAFFE && cfg->roi_bin_rule != MPN_ROI_BINS_ADAPTIVE) { set_error("mpn_frcnn_config.roi_bin_rule: %d is not an MPN_ROI_BINS_* value", cfg->roi_bin_rule); return MPN_EINVAL; }
  for (int l = 0; !graph_net && l < cfg->n_conv; ++l) MPN_CHECK_ARG(a.conv_w[l] != nullptr);
  const int C = cfg->n_classes;
  if (a.n_integral < 1 || a.n_integral > MPN_MAX_INTEGRAL) {
    set_error("mpn_frcnn_create_integral: invalid argument: n_integral %d is outside 1..MPN_MAX_INTEGRAL (%d)", a.n_integral, MPN_MAX_INTEGRAL);
    return MPN_EINVAL;
  }
  if (a.n_integral > 1 && C > 256) {
    set_error("mpn_frcnn_create_integral: invalid argument: %d integral classifiers need n_classes <= 256 (the integral score kernel's limit), not %d", a.n_integral, C);
    return MPN_EINVAL;
  }
  if (const mpn_mpnet_weights *mw = a.mw) {
    MPN_CHECK_ARG(mw->n_towers >= 2 && mw->n_towers <= 8 && mw->tap_conv3 >= 0 && mw->tap_conv4 > mw->tap_conv3 && mw->tap_conv4 < cfg->n_conv - 1);
    MPN_CHECK_ARG(C <= 256 && cfg->fc_dim % 128 == 0);
    MPN_CHECK_ARG(cfg->conv_cout[mw->tap_conv4] % 8 == 0 && cfg->conv_cout[mw->tap_conv3] % 8 == 0);
    for (int t = 0; t < mw->n_towers; ++t)
      MPN_CHECK_ARG(mw->region[t] >= 0 && mw->region[t] < 4 && mw->mix_w[t] && mw->fc6_w[t] && mw->fc7_w[t]);
  } else if (a.tower_heads() > 1) {
    const int *region = a.rw ? a.rw->head_region : a.gw->head_region;
    MPN_CHECK_ARG(C <= 256 && a.tower_heads() <= 8);
    for (int t = 0; t < a.tower_heads(); ++t) MPN_CHECK_ARG(region[t] >= 0 && region[t] < 4);
  }
  const int n_it = cfg->num_iter > 1 ? cfg->num_iter : 1;
  MPN_CHECK_ARG((size_t)n_it * cfg->max_rois <= MPN_NMS_MAX_BOXES);
  MPN_CHECK_ARG(!cfg->use_rbox_scores || n_it > 1);  // Tester_FRCNN.lua:92 assert(#all_output > 1)
  return MPN_OK;
}

// the conv layers' packed / Winograd / K = 36 weights, one C8P buffer per layer output, the MultiPathNet maps' range-max tables
static int build_vgg_trunk(mpn_frcnn *p, const CreateArgs &a) {
  const mpn_mpnet_weights *mw = a.mw;
  const int n_conv = p->cfg.n_conv;
  int h = p->cfg.max_h, w = p->cfg.max_w, cin = 3;
  size_t b = act_bytes(3, h, w);
  TRY(p->own.alloc(&p->img_c8p, b, true));
  p->act_bufs.push_back({p->img_c8p, b});
  for (int l = 0; l < n_conv; ++l) {
    ConvLayer L;
    L.Cin = cin; L.Cout = p->cout[l]; L.pool = p->pool_after[l];
    TRY(p->own.alloc(&L.wpk, conv_wpk_elems(L.Cin, L.Cout) * sizeof(float)));
    TRY(p->own.alloc(&L.bpk, (size_t)conv_coutp(L.Cout) * sizeof(float)));
    TRY(pack_conv_weights(a.conv_w[l], a.conv_b[l], L.Cin, L.Cout, L.wpk, L.bpk, nullptr));
    if (L.Cin <= 4 && !L.pool && !(mw && (l == mw->tap_conv3 || l == mw->tap_conv4))) {
      TRY(p->own.alloc(&L.w36, conv_first_elems(L.Cout) * sizeof(float)));
      TRY(pack_conv_weights_first(a.conv_w[l], L.Cin, L.Cout, L.w36, nullptr));
    }
    if (L.Cin >= 16) {  // fewer input channels: direct kernels (the 3-channel first layer is bound by its output stores either way)
      TRY(p->own.alloc(&L.wino, conv_wino_elems(L.Cin, L.Cout) * sizeof(float)));
      TRY(pack_conv_weights_wino(a.conv_w[l], L.Cin, L.Cout, L.wino, nullptr));
    }
    b = act_bytes(L.Cout, h, w);
    TRY(p->own.alloc(&L.out, b, true));
    p->act_bufs.push_back({L.out, b});
    if (mw && (l == mw->tap_conv3 || l == mw->tap_conv4 || l == n_conv - 1)) {  // range-max tables of the maps the towers pool
      const int slot = l == n_conv - 1 ? 0 : (l == mw->tap_conv4 ? 1 : 2);
      TRY(p->own.alloc(&p->vmax_tab[slot], (size_t)(vmax_levels_for(h) + 1) * b));  // levels 1..L (C8P form) or 0..L (pixel-major form)
    }
    if (L.pool) {
      h = (h + 1) / 2; w = (w + 1) / 2;
      b = act_bytes(L.Cout, h, w);
      TRY(p->own.alloc(&L.pooled, b, true));
      p->act_bufs.push_back({L.pooled, b});
    }
    cin = L.Cout;
    p->conv.push_back(L);
  }
  p->feat_c = cin;
  return MPN_OK;
}

// ResNet / op-list graph: the graph object owns the trunk and per-ROI weights and activations; the cls + bbox heads read its pooled vector
static int build_graph_net(mpn_frcnn *p, const CreateArgs &a) {
  const mpn_frcnn_config &c = p->cfg;
  if (a.rw) TRY(resnet_build(a.rw, c.max_h, c.max_w, c.max_rois, c.pooled_h, &p->rn));
  else TRY(graph_build(a.gw, c.max_h, c.max_w, c.max_rois, c.pooled_h, &p->rn));
  p->feat_c = resnet_feat_channels(p->rn);
  resnet_set_roi_bins(p->rn, c.roi_bin_rule);
  p->cfg.fc_dim = resnet_out_channels(p->rn);
  return MPN_OK;
}

// MultiPathNet (models/multipathnet.lua:64-120): the towers' mix / fc6 / fc7 weights, and which pair of them shares one pooled operand
static int build_mpnet_towers(mpn_frcnn *p, const CreateArgs &a) {
  const mpn_mpnet_weights *mw = a.mw;
  const int PP = p->cfg.pooled_h * p->cfg.pooled_w, F = p->cfg.fc_dim;
  const int c5 = p->feat_c, c4 = p->cout[p->tap4], c3 = p->cout[p->tap3];
  for (int t = 0; t < mw->n_towers; ++t) {
    mpn_frcnn::Tower T{};
    T.region = mw->region[t]; T.use4 = mw->use_conv4[t]; T.use3 = mw->use_conv3[t];
    T.total_feat = c5 + (T.use4 ? c4 : 0) + (T.use3 ? c3 : 0);
    TRY(pack_linear(p, mw->mix_w[t], mw->mix_b[t], T.total_feat, c5, 1, &T.mix_w, &T.mix_b));
    TRY(pack_linear(p, mw->fc6_w[t], mw->fc6_b[t], p->K6, F, PP, &T.w6, &T.b6));
    TRY(pack_linear(p, mw->fc7_w[t], mw->fc7_b[t], F, F, 1, &T.w7, &T.b7));
    if (p->cfg.fc_arith == MPN_FC_SPLIT3) {  // the towers' fc6 / fc7 weights as three bf16 planes
      TRY(pack_split3(p, T.w6, p->K6, F, &T.w6_s3));
      TRY(pack_split3(p, T.w7, F, F, &T.w7_s3));
    }
    p->towers.push_back(T);
  }
  for (int a_ = 0; a_ < (int)p->towers.size() && p->share_provider < 0; ++a_)      // the first (provider, consumer) pair, if any
    for (int b = 0; b < (int)p->towers.size() && p->share_provider < 0; ++b) {
      const mpn_frcnn::Tower &A = p->towers[a_], &B = p->towers[b];
      if (a_ == b || A.region != B.region || A.total_feat <= B.total_feat) continue;
      int la[3], lb[3], na = 0, nb = 0;   // the towers' map lists in concat order (conv345Combine: conv5, [conv4], [conv3])
      la[na++] = 0; if (A.use4) la[na++] = 1; if (A.use3) la[na++] = 2;
      lb[nb++] = 0; if (B.use4) lb[nb++] = 1; if (B.use3) lb[nb++] = 2;
      bool prefix = nb <= na;
      for (int i = 0; prefix && i < nb; ++i) prefix = la[i] == lb[i];
      if (prefix) { p->share_provider = a_; p->share_consumer = b; }
    }
  return MPN_OK;
}

// MultiPathNet: the towers' pooled operands and mix / fc6 outputs of both lanes, the pooling events (the pooling stream is `side`: build_streams)
static int build_mpnet_operands(mpn_frcnn *p) {
  const int PP = p->cfg.pooled_h * p->cfg.pooled_w, F = p->cfg.fc_dim, c5 = p->feat_c;
  int max_feat = 0;
  for (const mpn_frcnn::Tower &T : p->towers) max_feat = std::max(max_feat, T.total_feat);
  const size_t rows = (size_t)PP * p->Mp;
  const size_t tx_bytes = (size_t)(round_up(max_feat, 64) / 8) * rows * 8 * sizeof(float);
  const size_t ty_bytes = (size_t)(lin_np(c5) / 8) * rows * 8 * sizeof(float), tz_bytes = (size_t)(lin_np(F) / 8) * p->Mp * 8 * sizeof(float);
  TRY(p->own.alloc(&p->mix_scale, (size_t)3 * 3 * p->Mp * sizeof(float), true));
  TRY(p->own.alloc(&p->tx2, tx_bytes, true));
  if (p->share_provider >= 0) TRY(p->own.alloc(&p->tx3, tx_bytes, true));
  p->pool_on_side = true;
  for (int i = 0; i < 3; ++i) { TRY(p->own.event(&p->ev_pool_done[i])); TRY(p->own.event(&p->ev_mix_done[i])); }
  TRY(p->own.event(&p->ev_pool_go));
  TRY(p->own.alloc(&p->tx, tx_bytes, true));
  TRY(p->own.alloc(&p->ty, ty_bytes, true));
  TRY(p->own.alloc(&p->tz6, tz_bytes, true));
  if (p->cfg.fc_arith == MPN_FC_SPLIT3)
    for (int ln = 0; ln < 2; ++ln) {
      TRY(p->own.alloc(&p->ty_s3[ln], split3_plane_elems(p->K6, p->Mp) * sizeof(unsigned short), true));
      TRY(p->own.alloc(&p->tz6_s3[ln], split3_plane_elems(F, p->Mp) * sizeof(unsigned short), true));
    }
  TRY(p->own.alloc(&p->ty2, ty_bytes, true));  // the second tower lane
  return p->own.alloc(&p->tz6_2, tz_bytes, true);
}

// The integral classifier stage (model_utils.lua:296-313) behind `n_towers` towers, MultiPathNet's and the ResNet / op-list towers' alike:
// K classifiers on the Foveal towers' concat, the bbox regressor on tower 0, the concat and row-major outputs, the second lane's stream.
static int build_integral_classifier(mpn_frcnn *p, const CreateArgs &a, int n_towers, bool second_lane) {
  const int C = p->cfg.n_classes, F = p->cfg.fc_dim, n_fov = n_towers - 1, K = p->n_integral;
  const size_t M = p->cfg.max_rois;
  TRY(pack_linear(p, a.cls_w, a.cls_b, n_fov * F, K * C, 1, &p->wcls, &p->bcls));
  TRY(pack_linear(p, a.bbox_w, a.bbox_b, F, 4 * C, 1, &p->wbbox, &p->bbbox));
  TRY(p->own.alloc(&p->fov, M * 20 * sizeof(float), true));
  if (p->is_mpnet) TRY(build_mpnet_operands(p));  // here, between fov and cat: create's allocation order is kept as it was
  TRY(p->own.alloc(&p->cat, (size_t)n_towers * (lin_np(F) / 8) * p->Mp * 8 * sizeof(float), true));
  TRY(p->own.alloc(&p->cls_rm, M * K * C * sizeof(float), true));
  TRY(p->own.alloc(&p->bbox_rm, M * 4 * C * sizeof(float), true));
  if (second_lane) {
    TRY(p->own.stream(&p->tower_stream));
    TRY(p->own.event(&p->ev_lane_go));
    TRY(p->own.event(&p->ev_lane_done));
  }
  return MPN_OK;
}

// The plain Fast R-CNN head: fc6, fc7 (VGG trunks; a graph net ends in its own per-ROI stage), the fused cls + bbox GEMM, x6 / y6 / y7 / head,
// the final map's pixel-major copy.  *tmp_w / *tmp_b: the concatenated head weights, which the caller frees once packing has completed.
static int build_plain_head(mpn_frcnn *p, const CreateArgs &a, float **tmp_w, float **tmp_b) {
  const bool graph_net = a.graph_net(), split3 = p->cfg.fc_arith == MPN_FC_SPLIT3;
  const int PP = p->cfg.pooled_h * p->cfg.pooled_w, C = p->cfg.n_classes, F = p->cfg.fc_dim;
  const int KC = p->n_integral * C, NH = plain_head_width(p);  // the K classifiers' rows (K = 1 but for mpn_frcnn_create_integral); the fused head's
  const size_t M = p->cfg.max_rois, y_bytes = (size_t)(lin_np(F) / 8) * p->Mp * 8 * sizeof(float);
  if (!graph_net) {
    TRY(pack_linear(p, a.fc6_w, a.fc6_b, p->K6, F, PP, &p->w6, &p->b6));
    if (split3) {  // the weights' planes once, the operand's per image
      TRY(pack_split3(p, p->w6, p->K6, F, &p->w6_s3));
      TRY(p->own.alloc(&p->x6_s3, split3_plane_elems(p->K6, p->Mp) * sizeof(unsigned short), true));
    }
    TRY(pack_linear(p, a.fc7_w, a.fc7_b, F, F, 1, &p->w7, &p->b7));
    if (split3) {
      TRY(pack_split3(p, p->w7, F, F, &p->w7_s3));
      TRY(p->own.alloc(&p->y6_s3, split3_plane_elems(F, p->Mp) * sizeof(unsigned short), true));
    }
  }
  // cls (the K integral classifiers stacked) and bbox heads share their input -> one [(K+4)C, F] GEMM (model_utils.lua:105-119 ConcatTable)
  TRY(p->own.alloc(tmp_w, (size_t)NH * F * sizeof(float)));
  TRY(p->own.alloc(tmp_b, (size_t)NH * sizeof(float), true));
  hipError_t e = hipMemcpy(*tmp_w, a.cls_w, (size_t)KC * F * sizeof(float), hipMemcpyDeviceToDevice);
  if (e == hipSuccess) e = hipMemcpy(*tmp_w + (size_t)KC * F, a.bbox_w, (size_t)4 * C * F * sizeof(float), hipMemcpyDeviceToDevice);
  if (e == hipSuccess && a.cls_b) e = hipMemcpy(*tmp_b, a.cls_b, (size_t)KC * sizeof(float), hipMemcpyDeviceToDevice);
  if (e == hipSuccess && a.bbox_b) e = hipMemcpy(*tmp_b + KC, a.bbox_b, (size_t)4 * C * sizeof(float), hipMemcpyDeviceToDevice);
  if (e != hipSuccess) { set_error("mpn_frcnn_create: head weight copy failed: %s", hipGetErrorString(e)); return MPN_EHIP; }
  TRY(pack_linear(p, *tmp_w, *tmp_b, F, NH, 1, &p->wh, &p->bh));
  if (!graph_net) {
    int fh = p->cfg.max_h, fw = p->cfg.max_w;  // pixel-major copy of the final map at its largest size
    final_map_size(p, &fh, &fw);
    TRY(p->own.alloc(&p->up.pm, (size_t)fh * fw * ((p->feat_c + 7) / 8) * 8 * sizeof(float)));
    TRY(p->own.alloc(&p->x6, (size_t)(round_up(p->K6, 64) / 8) * p->Mp * 8 * sizeof(float), true));
    TRY(p->own.alloc(&p->y6, y_bytes, true));
  }
  TRY(p->own.alloc(&p->y7, y_bytes, true));
  return p->own.alloc(&p->head, M * NH * sizeof(float), true);
}

// rois, score / box tables, the iterative-localisation tables, the two NMS buffer sets
static int build_tail(mpn_frcnn *p) {
  const mpn_frcnn_config &c = p->cfg;
  const size_t M = c.max_rois, C = c.n_classes;
  TRY(p->own.alloc(&p->rois, M * 5 * sizeof(float), true));
  TRY(p->own.alloc(&p->scores, M * C * sizeof(float), true));
  TRY(p->own.alloc(&p->bbox, M * 4 * C * sizeof(float), true));
  TRY(p->own.alloc(&p->bbox_raw, M * 4 * C * sizeof(float), true));
  const int n_it = p->cfg.num_iter = std::max(c.num_iter, 1);
  const size_t MR = M * n_it;  // rows that reach NMS per class
  if (n_it > 1) {
    TRY(p->own.alloc(&p->it_scores, MR * C * sizeof(float), true));
    TRY(p->own.alloc(&p->it_bbox, MR * 4 * C * sizeof(float), true));
    TRY(p->own.alloc(&p->it_boxes, M * 4 * sizeof(float), true));
  }
  for (int i = 0; i < 2; ++i) {
    TRY(p->own.alloc(&p->scored_b[i], (C - 1) * MR * 5 * sizeof(float), true));
    TRY(p->own.alloc(&p->keep_b[i], (C - 1) * MR * 5 * sizeof(float), true));
    if (c.bbox_voting) TRY(p->own.alloc(&p->voted_b[i], (C - 1) * MR * 5 * sizeof(float), true));
    TRY(p->own.alloc(&p->keep_idx_b[i], (C - 1) * MR * sizeof(int), true));
    TRY(p->own.alloc(&p->counts_b[i], (C - 1) * sizeof(int), true));
    TRY(p->own.alloc(&p->n_keep_b[i], (C - 1) * sizeof(int), true));
    TRY(p->own.alloc(&p->thresh_b[i], 16, true));
  }
  p->scored = p->scored_b[0]; p->keep = p->keep_b[0]; p->keep_idx = p->keep_idx_b[0];
  p->counts = p->counts_b[0]; p->n_keep = p->n_keep_b[0]; p->thresh = p->thresh_b[0];
  return MPN_OK;
}

// The side stream (NMS / top-k tail under the next image's trunk) has the DEFAULT priority since round 5.  Rounds 1-4 created it with
// the highest one; what that bought the headline is nothing measurable (3.457-3.476 ms either way, six alternating runs), and what it can
// cost is large: a priority stream lands in a different hardware-queue class, and depending on which queue HIP's round-robin hands it,
// EVERY dispatch of the launch queue took 30-50 us longer while the two queues were both active — a mixed-size stream inside bench.py ran
// at 4.59 ms per image with the highest priority, 4.05 with the lowest, 3.12 with the default (profiles/r05_mixed_sizes_timeline.txt).
static int build_streams(mpn_frcnn *p) {
  TRY(p->own.stream(&p->side));
  for (int i = 0; i < 2; ++i) { TRY(p->own.event(&p->ev_head[i])); TRY(p->own.event(&p->ev_tail[i])); }
  if (p->pool_on_side) p->pool_stream = p->side;
  return MPN_OK;
}

static int create_handle(const CreateArgs &a, mpn_frcnn **out) {
  MPN_CHECK_ARG(out != nullptr);
  TRY(check_config(a));
  const mpn_frcnn_config *cfg = a.cfg;
  std::unique_ptr<mpn_frcnn, decltype(&mpn_frcnn_destroy)> h(new mpn_frcnn(), mpn_frcnn_destroy);  // from here on every return destroys the handle and what it owns
  mpn_frcnn *p = h.get();
  p->cfg = *cfg;
  p->create_scale_target = cfg->scale_target;
  {  // captured launch graphs: OFF unless asked for (MPN_GRAPHS=1 in the environment, or mpn_frcnn_set_graphs per handle).  Measured on
     // MI355X (profiles/r04_launch_graphs.txt): the host's enqueue time per AlexNet image drops 484 -> 74 us, but the device-side timeline
     // does not change (the gaps between dependent kernels are the command processor's, not the host's) and the throughput lines read
     // 0.5 % LOWER with replays (c2 287.2 vs 289.1 k, c1 373.9 vs 376.4 k proposals/s): a host-CPU saving, not a speed-up, so it is opt-in
    const char *e = getenv("MPN_GRAPHS");
    if (e && (e[0] == '0' || e[0] == '1')) p->graphs_on = e[0] == '1';
  }
  if (hipGetDevice(&p->device) != hipSuccess) { set_error("mpn_frcnn_create: no current HIP device"); return MPN_EHIP; }
  p->scratch.device = p->device;
  ScratchScope scratch_scope(&p->scratch);
  const bool graph_net = a.graph_net();
  const int tower_heads = a.tower_heads();
  if (tower_heads > 1) p->n_integral = (a.rw ? a.rw->n_integral : a.gw->n_integral) > 0 ? (a.rw ? a.rw->n_integral : a.gw->n_integral) : 1;
  if (const mpn_mpnet_weights *mw = a.mw) { p->is_mpnet = true; p->tap3 = mw->tap_conv3; p->tap4 = mw->tap_conv4; p->n_integral = mw->n_integral > 0 ? mw->n_integral : 1; p->conv345_norm = !mw->conv345_unnormalized; }
  if (!a.mw && !graph_net) p->n_integral = a.n_integral;  // mpn_frcnn_create_integral: K classifiers in the plain head
  const int n_conv = graph_net ? 0 : cfg->n_conv;
  p->cfg.n_conv = n_conv;
  if (n_conv) { p->cout.assign(cfg->conv_cout, cfg->conv_cout + n_conv); p->pool_after.assign(cfg->pool_after, cfg->pool_after + n_conv); }
  p->cfg.conv_cout = p->cout.data();
  p->cfg.pool_after = p->pool_after.data();
  TRY(build_vgg_trunk(p, a));
  if (graph_net) TRY(build_graph_net(p, a));
  MPN_CHECK_ARG(p->feat_c % 8 == 0);
  p->K6 = p->feat_c * cfg->pooled_h * cfg->pooled_w;
  p->Mp = lin_mp(cfg->max_rois);
  p->n_head = 5 * cfg->n_classes;
  float *tmp_w = nullptr, *tmp_b = nullptr;
  if (a.mw) {
    TRY(build_mpnet_towers(p, a));
    TRY(build_integral_classifier(p, a, a.mw->n_towers, true));
  } else if (tower_heads > 1) {  // ResNet / graph towers (this library's extension, see mpn_resnet_weights): same classifier stage as MultiPathNet
    const int *region = a.rw ? a.rw->head_region : a.gw->head_region;
    p->rn_region.assign(region, region + tower_heads);
    TRY(build_integral_classifier(p, a, tower_heads, resnet_has_second_lane(p->rn)));  // (that lane: debug flavour only)
  } else {
    TRY(build_plain_head(p, a, &tmp_w, &tmp_b));
  }
  TRY(build_tail(p));
  TRY(build_streams(p));
  const hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) { set_error("mpn_frcnn_create: %s", hipGetErrorString(e)); return MPN_EHIP; }
  for (float **q : {&tmp_w, &tmp_b}) p->own.free_now(q);  // the pack kernels have run: nothing reads the concatenated head weights again
  *out = h.release();
  return MPN_OK;
}
#undef TRY

// The trunk on an H x W image into the record `m` (the map goes to m->buf if set) — the only record it touches: invalid from the
// start, valid again where the last launch is enqueued.  Hc > 0: the image is one level of an image pyramid, placed top-left in a
// zero Hc x Wc canvas on which the whole trunk runs (getImages' padded batch, ImageDetect.lua:44-49).
static int run_trunk(mpn_frcnn *p, const float *d_image, int H, int W, hipStream_t s, mpn_frcnn::CachedMap *m, int Hc = 0, int Wc = 0) {
  const mpn_frcnn_config &c = p->cfg;
  float *const final_out = m->buf;
  m->invalidate();
  const bool canvas = Hc > 0;
  if (!canvas) { Hc = H; Wc = W; }
  if (Hc != p->last_h || Wc != p->last_w) {  // halo positions move with the image size: re-lay the zero halo of every activation, once
    if (g_halo_memset) {
      for (auto &b : p->act_bufs) MPN_CHECK_HIP(hipMemsetAsync(b.first, 0, b.second, s));
    } else {
      std::vector<Act> acts;
      acts.push_back(make_act(p->img_c8p, 3, Hc, Wc));
      int hh = Hc, ww = Wc;
      for (auto &L : p->conv) {
        if (L.out) acts.push_back(make_act(L.out, L.Cout, hh, ww));
        if (L.pool) { hh = (hh + 1) / 2; ww = (ww + 1) / 2; if (L.pooled) acts.push_back(make_act(L.pooled, L.Cout, hh, ww)); }
      }
      int rc_h = c8p_zero_halos(acts.data(), (int)acts.size(), s);
      if (rc_h) return rc_h;
    }
    p->last_h = Hc; p->last_w = Wc;
  }
  Act cur = make_act(p->img_c8p, 3, Hc, Wc);
  p->vmax_built[0] = p->vmax_built[1] = p->vmax_built[2] = false;
  int rc;
  { ProfScope ps(p, MPN_PROF_TRANSFORM, s);
    rc = canvas ? image_transform_canvas_c8p(d_image, H, W, c.tf_swap, c.tf_scale, c.tf_mean, c.tf_std, c.tf_std[0] != 0.0, cur, s)
                : image_transform_c8p(d_image, H, W, c.tf_swap, c.tf_scale, c.tf_mean, c.tf_std, c.tf_std[0] != 0.0, cur, s); }
  if (rc) return rc;
  int h = Hc, w = Wc;
  int li = 0;
  for (auto &L : p->conv) {
    float *const final_here = (final_out && &L == &p->conv.back()) ? final_out : nullptr;
    Act out = make_act(final_here && !L.pool ? final_here : L.out, L.Cout, h, w);
    const int ctag = conv3x3_variant_for(L.Cout, L.wino != nullptr) == 7 ? MPN_PROF_CONV_WINO : MPN_PROF_CONV_DIRECT;
    const bool is_tap = p->is_mpnet && (li == p->tap3 || li == p->tap4);
    const bool keep_out = is_tap || (p->keep_prepool_from >= 0 && li >= p->keep_prepool_from);  // a training image: the backward pass reads the pre-pool map
    if (is_tap) p->tap_act[li == p->tap4 ? 1 : 2] = out;
    ++li;
    if (L.pool) {
      Act pooled = make_act(final_here ? final_here : L.pooled, L.Cout, (h + 1) / 2, (w + 1) / 2);
      if (g_fuse_pool) {
        ProfScope ps(p, ctag, s);
        rc = conv3x3_c8p(cur, L.wpk, L.bpk, L.Cout, 1, keep_out ? out : Act{}, pooled, s, L.wino);  // tap layers keep the pre-pool map too
      } else {
        { ProfScope ps(p, ctag, s); rc = conv3x3_c8p(cur, L.wpk, L.bpk, L.Cout, 1, out, Act{}, s, L.wino); }
        if (rc == MPN_OK) { ProfScope ps(p, MPN_PROF_POOL, s); rc = maxpool2x2_c8p(out, pooled, s); }
      }
      if (rc) return rc;
      cur = pooled; h = pooled.H; w = pooled.W;
    } else {
      { ProfScope ps(p, ctag, s);
        rc = (L.w36 && g_first_k36) ? conv3x3_first_c8p(cur, L.w36, L.bpk, L.Cout, 1, out, s) : conv3x3_c8p(cur, L.wpk, L.bpk, L.Cout, 1, out, Act{}, s, L.wino); }
      if (rc) return rc;
      cur = out;
    }
  }
  m->act = cur; m->h = H; m->w = W;
  return MPN_OK;
}

// One fc6 / fc7 layer (Linear + ReLU) x[N, K] -> y[N, fc_dim] on C8 operands, timed under `tag`: the fp32 GEMM, or where the layer has
// w_s3 (MPN_FC_SPLIT3) the operand split into three bf16 planes (x_s3), then six bf16 products per k-step with fp32 accumulation, fixed K ranges
static int fc_relu(mpn_frcnn *p, int tag, const float *x, int N, int K, const float *w, const float *b, const unsigned short *w_s3,
                   unsigned short *x_s3, float *y, hipStream_t s, int Mp_override) {
  ProfScope ps(p, tag, s);
  if (!w_s3) return linear_c8(x, N, K, w, b, p->cfg.fc_dim, 1, y, nullptr, s, Mp_override, nullptr, 1);
  const int rc = split3_planes(x, K, lin_mp(N), lin_mp(N), x_s3, s);
  return rc ? rc : linear_c8_split3(x_s3, N, K, w_s3, b, p->cfg.fc_dim, 1, y, s);
}

// models/multipathnet.lua:64-120 + model_utils.lua:209-251,296-313 on the C8 layouts: Foveal -> per tower
// {ROI pools of conv5 / conv4 / conv3 written side by side = the channel concat, per-map L2 normalise * 1000,
// 1x1 conv mix as a GEMM over (bin, roi) rows whose output IS the fc6 operand, fc6, fc7 into the tower concat}
// -> K integral classifiers (mean of softmaxes) + bbox regressor on the "het" tower.
static int run_integral_heads(mpn_frcnn *p, const float *d_boxes, int N, int H, int W, int n_fov, hipStream_t s, int clamp);

static int run_mpnet_head(mpn_frcnn *p, const Act &conv5, const float *d_boxes, int N, int H, int W, hipStream_t s, int clamp) {
  const mpn_frcnn_config &c = p->cfg;
  const int F = c.fc_dim, PP = c.pooled_h * c.pooled_w, Mp = lin_mp(N);
  int rc = mpn_foveal_forward(p->rois, N, p->fov, s);
  if (rc) return rc;
  const Act maps[3] = {conv5, p->tap_act[1], p->tap_act[2]};
  const float scales[3] = {c.spatial_scale, c.spatial_scale * 2.0f, c.spatial_scale * 4.0f};
  const float kConv345Factor[3] = {1.0f, (float)(1.0 / 30), (float)(1.0 / 200)};  // model_utils.lua:231-237 normFactor (Lua doubles -> float)
  const int Fcb = lin_np(F) / 8;
  const bool pm = g_roi_pool_pm != 0;  // pixel-major range-max tables + fused sum of squares (round 3); 0 = the C8P form (test hook)
  // The range-max tables: once per trunk run and map (iterative localisation on the cached maps reuses them).  Round 6: with the pooling
  // stream, a map's tables are built THERE, where the first pooling that reads them is enqueued — the first tower in execution order pools
  // conv5 alone (cheapest first), so only conv5's small tables (1/7 of the bytes) stand between the trunk and the first GEMM; conv4's and
  // conv3's levels (HBM-bound writes) are built under that tower's GEMMs instead of in front of everything.
  if (p->vmax_pm != pm) { p->vmax_built[0] = p->vmax_built[1] = p->vmax_built[2] = false; p->vmax_pm = pm; }
  auto build_tables = [&](int m, hipStream_t st) -> int {
    if (p->vmax_built[m]) return MPN_OK;
    ProfScope ps(p, MPN_PROF_ROIPOOL, st);
    const int rcb = pm ? build_vmax_tables_pm(maps[m], p->vmax_tab[m], st) : build_vmax_tables(maps[m], p->vmax_tab[m], st);
    if (rcb == MPN_OK) p->vmax_built[m] = true;
    return rcb;
  };
  // nn.Normalize's per-(ROI, map) scale folded into the mix GEMM (linear_c8_rowscaled).  Fold or in-place l2norm_apply is decided by
  // the network alone (channel counts), never by the ROI count, and the mix GEMM — K = the channel concat, >= 49 row tiles for any N —
  // always runs as ONE un-split accumulation chain, so a ROI's mix output does not depend on the rows it is batched with (ADVICE r3:
  // a 128-row shard of a feat_c <= 256 trunk used to take l2norm_apply + split-K where the full table took the fold)
  const bool fold_scale = pm && p->conv345_norm && p->mix_scale && g_mix_fold &&
                          maps[0].C % 32 == 0 && maps[1].C % 32 == 0 && maps[2].C % 32 == 0;  // segment boundaries fall on 32-k stages
  // Two streams: a tower's skip pooling is L2 -> L1 bound (no matrix work), its GEMMs are matrix-bound, and the folding GEMM leaves
  // half of every CU's registers and 94 KB of LDS free.  Tower t's pooling therefore runs on the handle's pooling stream, into the
  // operand buffer / scale set of parity t & 1, under tower t - 1's GEMMs on `s`; `s` waits for the pooling only where the mix GEMM
  // starts, the pooling stream waits for the mix GEMM of tower t - 2 (the previous user of its buffers).  Every result is still
  // ordered on `s`.  (Profiling scopes time each stream's own work; with overlap their sum exceeds the wall time.)
  // Rows of the pooled operand = the mix GEMM's rows = (bin, roi).  With the scale fold (the product path) they are PACKED: Nr = N rounded up to 8
  // rows per bin instead of the Mp = N rounded up to 128 the fc GEMMs' operands carry, and the mix GEMM scatters its output rows into fc6's
  // [cout block][bin][Mp][8] operand (GemmArgs::bin_rows).  1000 proposals: 49 x 1000 = 383 row tiles instead of 49 x 1024 = 392 — 1532 blocks
  // instead of 1568 on 512 resident slots, i.e. 2.99 rounds instead of 3.06 (a whole block time per mix GEMM); 300 proposals: 115 instead of 147.
  const int Nr = (fold_scale && g_mix_packed) ? round_up(N, 8) : Mp;
  const int R = PP * Nr, Rp = round_up(R, 128);
  const bool overlap = pm && p->pool_stream && p->tx2 && g_pool_overlap;
  hipStream_t ps_stream = overlap ? p->pool_stream : s;
  if (!(overlap && g_tables_lazy))   // one stream (or the round-3..5 order, hook tables_lazy = 0): all tables up front
    for (int m = 0; m < 3; ++m) if ((rc = build_tables(m, s)) != MPN_OK) return rc;
  if (overlap) {  // the tables, the Foveal regions and everything before them on `s`
    MPN_CHECK_HIP(hipEventRecord(p->ev_pool_go, s));
    MPN_CHECK_HIP(hipStreamWaitEvent(ps_stream, p->ev_pool_go, 0));
  }
  const int n_tow = (int)p->towers.size();
  MPN_CHECK_ARG(n_tow <= 8);
  // ---- the operand plan of this image: which pooled-operand buffer each tower's mix GEMM reads, and which tower's arrival pools it.
  // Plain towers alternate between tx and tx2 (buffers 0 / 1); the (provider, consumer) pair of mpn_frcnn::share_provider shares tx3
  // (buffer 2): whichever of the two comes first pools the PROVIDER's maps there, the other one finds them.  prev_user = the tower whose
  // mix GEMM read the buffer last (its ev_mix_done is what a re-pooling waits for; by construction it is at least two towers back, so
  // its mix GEMM has been enqueued whenever the pooling is).
  const bool share = overlap && p->tx3 && p->share_provider >= 0 && g_tower_share;
  float *const tx_of[3] = {p->tx, p->tx2, p->tx3};
  int buf_of[8], prev_user[8], pool_src[8], order[8];
  bool pools[8];
  // Execution order: the towers meet only in `cat` (each writes its own slice), so the order is free — cheapest pooling first.  The first
  // tower's pooling has nothing to hide behind (it follows the trunk directly): 512 channels (the conv5-only tower) instead of 1280.
  for (int t = 0; t < n_tow; ++t) order[t] = t;
  if (overlap && g_tower_order) {
    auto cost = [&](int t) { return (share && (t == p->share_provider || t == p->share_consumer)) ? p->towers[p->share_provider].total_feat : p->towers[t].total_feat; };
    std::stable_sort(order, order + n_tow, [&](int x, int y) { return cost(x) < cost(y); });
  }
  {
    int nplain = 0, last_user[3] = {-1, -1, -1};
    bool shared_pooled = false;
    for (int k = 0; k < n_tow; ++k) {
      const int t = order[k];
      if (share && (t == p->share_provider || t == p->share_consumer)) {
        buf_of[t] = 2; pools[t] = !shared_pooled; shared_pooled = true; pool_src[t] = p->share_provider;
      } else {
        buf_of[t] = overlap ? (nplain & 1) : 0; ++nplain; pools[t] = true; pool_src[t] = t;
      }
      prev_user[t] = pools[t] ? last_user[buf_of[t]] : -1;
      last_user[buf_of[t]] = t;
    }
  }
  GemmRowScale grs_of[8];
  for (int t = 0; t < n_tow; ++t) {  // the per-(map, ROI) scale vectors tower t's mix GEMM applies: those of its buffer, its own K segments
    const mpn_frcnn::Tower &T = p->towers[t];
    GemmRowScale &grs = grs_of[t];
    grs = GemmRowScale{};
    grs.rs_mod = Nr;
    if (!fold_scale) continue;
    if (Nr != Mp) { grs.bin_rows = Nr; grs.out_Mp = Mp; grs.x_pitch = R; }
    const int used[3] = {1, T.use4, T.use3};
    int cb_off = 0;
    for (int m = 0; m < 3; ++m) {
      if (!used[m]) continue;
      grs.scale[grs.n_seg] = p->mix_scale + ((size_t)buf_of[t] * 3 + grs.n_seg) * p->Mp;
      if (grs.n_seg < 2) grs.k_end[grs.n_seg] = (cb_off + maps[m].Cb()) * 8;
      ++grs.n_seg;
      cb_off += maps[m].Cb();
    }
  }
  auto pool_tower = [&](int t) -> int {  // pooling (+ normalisation scales) of tower t's operand on the pooling stream
    if (!pools[t]) return MPN_OK;          // the other tower of the shared pair pooled it
#ifdef MPN_DEBUG_HOOKS
    if (g_mpn_pool_knock) {                // mpn_debug_set_mpn_pool_knock (timing only, stale operands): what the skip pooling costs the towers' GEMMs
      if (overlap) MPN_CHECK_HIP(hipEventRecord(p->ev_pool_done[buf_of[t]], ps_stream));
      return MPN_OK;
    }
#endif
    const mpn_frcnn::Tower &T = p->towers[pool_src[t]];
    const int b = buf_of[t];
    float *txb = tx_of[b];
    const float *reg = p->fov + 5 * T.region;  // rows 4n + region of the Foveal table
    if (overlap && prev_user[t] >= 0) MPN_CHECK_HIP(hipStreamWaitEvent(ps_stream, p->ev_mix_done[b], 0));  // the buffer's last reader
    int cb_off = 0, seg = 0;
    const int used[3] = {1, T.use4, T.use3};
    int rcl = MPN_OK;
    for (int m = 0; m < 3; ++m) {
      if (!used[m]) continue;
      float *dst = txb + (size_t)cb_off * R * 8;
      if ((rcl = build_tables(m, ps_stream)) != MPN_OK) return rcl;   // (first reader of the map's tables this trunk run)
      { ProfScope ps(p, MPN_PROF_ROIPOOL, ps_stream);
        if (pm) {
          float *sc_out = fold_scale ? p->mix_scale + ((size_t)b * 3 + seg) * p->Mp : nullptr;
          rcl = roi_pool_pm_rmq(maps[m], p->vmax_tab[m], reg, N, c.pooled_h, c.pooled_w, scales[m], RoiRule{1.0f, 0, c.roi_bin_rule}, dst, ps_stream, 20, Nr, p->conv345_norm ? 1 : 0,
                                p->conv345_norm ? 1000.0f : kConv345Factor[m], sc_out);
          ++seg;
        } else {
          rcl = roi_pool_c8_rmq(maps[m], p->vmax_tab[m], reg, N, c.pooled_h, c.pooled_w, scales[m], RoiRule{1.0f, 0, c.roi_bin_rule}, dst, ps_stream, 20, Nr);
          if (rcl == MPN_OK) rcl = p->conv345_norm ? l2norm_scale_c8(dst, maps[m].Cb() * PP, Nr, N, 1000.0f, ps_stream)
                                                   : mul_const_c8(dst, maps[m].Cb() * PP, Nr, N, kConv345Factor[m], ps_stream);
        } }
      if (rcl) return rcl;
      cb_off += maps[m].Cb();
    }
    if (overlap) MPN_CHECK_HIP(hipEventRecord(p->ev_pool_done[b], ps_stream));
    return MPN_OK;
  };
  // Two tower lanes (mpn_frcnn::tower_stream): tower ti runs on lane ti & 1 — its own stream, its own mix-output / fc6-output buffers.
  // The pooling stream runs one tower ahead of EACH lane (towers 0 and 1 up front, tower ti + 2 as soon as tower ti's mix GEMM is
  // enqueued).  The lanes join before the classifiers.  (profiling keeps one lane: its per-group scopes time the launch stream)
  const bool lanes = overlap && p->tower_stream && p->ty2 && p->tz6_2 && g_tower_lanes && n_tow > 1 && !p->prof;
  hipStream_t lane_s[2] = {s, lanes ? p->tower_stream : s};
  float *lane_ty[2] = {p->ty, lanes ? p->ty2 : p->ty}, *lane_tz6[2] = {p->tz6, lanes ? p->tz6_2 : p->tz6};
  if (lanes) {  // everything the towers read (Foveal regions, tables, the previous image's use of the lane buffers) is ordered on `s`
    MPN_CHECK_HIP(hipEventRecord(p->ev_lane_go, s));
    MPN_CHECK_HIP(hipStreamWaitEvent(lane_s[1], p->ev_lane_go, 0));
  }
  rc = pool_tower(order[0]);
  if (rc) return rc;
  if (lanes) { rc = pool_tower(order[1]); if (rc) return rc; }
  for (int k = 0; k < n_tow; ++k) {
    const int ti = order[k];
    const mpn_frcnn::Tower &T = p->towers[ti];
    const int b = buf_of[ti];
    const int ln = lanes ? (k & 1) : 0;
    hipStream_t ls = lane_s[ln];
    SplitkSlotScope lane_slabs(ln ? SCR_GEMM_SPLITK_LANE : SCR_GEMM_SPLITK);  // a GEMM of few tiles (small ROI shards) runs split-K: each lane its own slabs
    const float *txb = tx_of[b];
    if (overlap) {
      MPN_CHECK_HIP(hipStreamWaitEvent(ls, p->ev_pool_done[b], 0));
      if (!lanes && k + 1 < n_tow) { rc = pool_tower(order[k + 1]); if (rc) return rc; }  // enqueued now: runs under this tower's GEMMs
    }
    const GemmRowScale &grs = grs_of[ti];
    // 1x1 conv mix: rows = (bin, roi), K = concat channels, N = feat_c; output layout == fc6 operand layout
    { ProfScope ps(p, MPN_PROF_HEADS, ls);
      rc = fold_scale ? linear_c8_rowscaled(txb, R, T.total_feat, T.mix_w, T.mix_b, p->feat_c, 0, lane_ty[ln], ls, Rp, grs)
                      : linear_c8(txb, PP * Mp, T.total_feat, T.mix_w, T.mix_b, p->feat_c, 0, lane_ty[ln], nullptr, ls, PP * Mp, nullptr, 2); }
    if (rc) return rc;
    if (overlap) MPN_CHECK_HIP(hipEventRecord(p->ev_mix_done[b], ls));
    if (lanes && k + 2 < n_tow) { rc = pool_tower(order[k + 2]); if (rc) return rc; }  // waits for its buffer's last reader; runs under this lane's fc6 and the other lane's tower
    rc = fc_relu(p, MPN_PROF_FC6, lane_ty[ln], N, p->K6, T.w6, T.b6, T.w6_s3, p->ty_s3[ln], lane_tz6[ln], ls, Mp);
    if (rc) return rc;
    rc = fc_relu(p, MPN_PROF_FC7, lane_tz6[ln], N, F, T.w7, T.b7, T.w7_s3, p->tz6_s3[ln], p->cat + (size_t)ti * Fcb * Mp * 8, ls, Mp);
    if (rc) return rc;
    if (!overlap && k + 1 < n_tow) { rc = pool_tower(order[k + 1]); if (rc) return rc; }
  }
  if (lanes) {
    MPN_CHECK_HIP(hipEventRecord(p->ev_lane_done, lane_s[1]));
    MPN_CHECK_HIP(hipStreamWaitEvent(s, p->ev_lane_done, 0));
  }
  return run_integral_heads(p, d_boxes, N, H, W, (int)p->towers.size() - 1, s, clamp);
}

// the stage after the towers (model_utils.lua:296-315, multipathnet.lua:112-120): K classifier clones on the concatenated
// classification towers -> mean of their softmaxes; box regressor on the last tower; decode + clamp
static int run_integral_heads(mpn_frcnn *p, const float *d_boxes, int N, int H, int W, int n_fov, hipStream_t s, int clamp) {
  const mpn_frcnn_config &c = p->cfg;
  const int C = c.n_classes, F = c.fc_dim, Mp = lin_mp(N), K = p->n_integral;
  const int Fcb = lin_np(F) / 8;
  int rc;
  { ProfScope ps(p, MPN_PROF_HEADS, s);
    rc = linear_c8(p->cat, N, n_fov * F, p->wcls, p->bcls, K * C, 0, nullptr, p->cls_rm, s, Mp, nullptr, 1);
    if (rc == MPN_OK) rc = linear_c8(p->cat + (size_t)n_fov * Fcb * Mp * 8, N, F, p->wbbox, p->bbbox, 4 * C, 0, nullptr, p->bbox_rm, s, Mp, nullptr, 1); }
  if (rc) return rc;
  ProfScope ps_post(p, MPN_PROF_POST, s);
  rc = launch_integral_softmax_mean(p->cls_rm, K * C, N, K, C, p->scores, s);
  if (rc) return rc;
  return launch_head_decode(p->bbox_rm, 4 * C, 0, N, C, d_boxes, c.bbox_mean, c.bbox_std, clamp, (float)W, (float)H, p->bbox_raw, p->bbox, s);
}

// getImages' rescaled image buffers (ImageDetect.lua:34-43), grown to hold `need` / `need_t` bytes
static int grow_scaled(mpn_frcnn *p, size_t need, size_t need_t, hipStream_t s) {
  const int rc = p->own.grow(&p->scaled, &p->scaled_bytes, need, s);
  return rc ? rc : p->own.grow(&p->scale_tmp, &p->scale_tmp_bytes, need_t, s);
}

// getImages with a scale table (ImageDetect.lua:22-52; include/mpn.h mpn_frcnn_set_scales): level l's image, resampled and transformed as
// the single-scale image is, top-left in a zero canvas of the largest level's size -> the whole trunk -> its final map into slot l.
// A level whose scale repeats an earlier one's is not recomputed (no ROI can pick it).  *feat: slot 0's view (every slot has its
// geometry).  d_image == nullptr: the maps of the last image are reused (iterative localisation).
static int run_pyramid_trunk(mpn_frcnn *p, const float *d_image, int H0, int W0, hipStream_t s, Act *feat) {
  const mpn_frcnn_config &c = p->cfg;
  const int S = p->n_scales;
  double sc[MPN_MAX_SCALES];
  int hl[MPN_MAX_SCALES], wl[MPN_MAX_SCALES], Hc = 0, Wc = 0;
  for (int l = 0; l < S; ++l) {
    sc[l] = getimages_size(H0, W0, p->scale_targets[l], c.scale_max, &hl[l], &wl[l]);
    if (hl[l] <= 0 || wl[l] <= 0) { set_error("run_detect: level %d of a %dx%d image is %dx%d", l, H0, W0, hl[l], wl[l]); return MPN_EINVAL; }
    Hc = std::max(Hc, hl[l]); Wc = std::max(Wc, wl[l]);
  }
  if (Hc > c.max_h || Wc > c.max_w) {
    set_error("run_detect: the %d-level pyramid of a %dx%d image needs a %dx%d canvas; the pipeline holds %dx%d", S, H0, W0, Hc, Wc, c.max_h, c.max_w);
    return MPN_EINVAL;
  }
  int fh = Hc, fw = Wc;
  final_map_size(p, &fh, &fw);
  *feat = make_act(p->ms_feat, p->feat_c, fh, fw);
  if (!d_image) {
    if (p->ms_h0 != H0 || p->ms_w0 != W0 || p->last_h != Hc || p->last_w != Wc) { set_error("run_detect: no cached pyramid for a %dx%d image", H0, W0); return MPN_ESTATE; }
    return MPN_OK;
  }
  p->ms_h0 = p->ms_w0 = -1;
  p->ms_pm_valid = false;
  p->up.invalidate();  // the levels run through the upright trunk's buffers
  size_t need = 0, need_t = 0;
  for (int l = 0; l < S; ++l)
    if (sc[l] != 1.0) { need = std::max(need, (size_t)3 * hl[l] * wl[l] * sizeof(float)); need_t = std::max(need_t, (size_t)3 * H0 * wl[l] * sizeof(float)); }
  int rc = grow_scaled(p, need, need_t, s);
  if (rc) return rc;
  for (int l = 0; l < S; ++l) {
    int src = l;
    for (int k = 0; k < l && src == l; ++k) if (sc[k] == sc[l]) src = k;
    p->ms_src[l] = src;
    p->ms_scales[l] = sc[l];
    if (src != l) continue;
    const float *img = d_image;
    if (sc[l] != 1.0) {
      rc = mpn_image_scale(d_image, 3, H0, W0, hl[l], wl[l], p->scale_tmp, p->scaled, s);
      if (rc) return rc;
      img = p->scaled;
    }
    mpn_frcnn::CachedMap level;  // (the pyramid keeps its own record of what is cached: ms_h0 / ms_w0)
    level.buf = p->ms_feat + (size_t)l * p->ms_slot;
    rc = run_trunk(p, img, hl[l], wl[l], s, &level, Hc, Wc);
    if (rc) return rc;
  }
  p->ms_h0 = H0; p->ms_w0 = W0;
  return MPN_OK;
}

// The features of a detect: *feat = the final map to pool from (ResNet / op-list handles keep theirs inside the graph object).  H x W: the
// network-input size of the H0 x W0 image at getImages' scale sc.  d_image == nullptr: recompute_features = false (ImageDetect.lua:107-111)
// — the last call's map is reused (iterative localisation, Tester_FRCNN.lua:82-89).  `m`: the VGG trunk's record to fill or to read.
int mpn::obtain_features(mpn_frcnn *p, const float *d_image, int H0, int W0, int H, int W, double sc, mpn_frcnn::CachedMap *m, hipStream_t s, Act *feat) {
  const mpn_frcnn_config &c = p->cfg;
  if (p->n_scales > 1) return run_pyramid_trunk(p, d_image, H0, W0, s, feat);  // getImages per level
  const float *img = d_image;
  if (d_image && sc != 1.0) {
    int rc = grow_scaled(p, (size_t)3 * H * W * sizeof(float), (size_t)3 * H0 * W * sizeof(float), s);
    if (rc) return rc;
    rc = mpn_image_scale(d_image, 3, H0, W0, H, W, p->scale_tmp, p->scaled, s);
    if (rc) return rc;
    img = p->scaled;
  }
  if (p->rn) {
    if (!d_image) {
      if (!resnet_has_features(p->rn, H, W)) { set_error("run_detect: no cached features for a %dx%d image", H0, W0); return MPN_ESTATE; }
      return MPN_OK;
    }
    ProfScope ps(p, MPN_PROF_CONV_DIRECT, s);
    return resnet_trunk_forward(p->rn, img, H, W, c.tf_swap, c.tf_scale, c.tf_mean, c.tf_std, c.tf_std[0] != 0.0, s);
  }
  if (!d_image) {
    if (m->h != H || m->w != W || p->last_h != H || p->last_w != W) {
      set_error("run_detect: no cached %sfeatures for a %dx%d image", m == &p->mir ? "mirrored " : "", H0, W0);
      return MPN_ESTATE;
    }
  } else {
    if (m == &p->up) p->mir.invalidate();  // a new upright map: the mirrored one of the last image no longer goes with it
    const int rc = run_trunk(p, img, H, W, s, m);
    if (rc) return rc;
  }
  *feat = m->act;
  return MPN_OK;
}

// ResNet towers: Foveal region t -> ROI pool -> layer4 copy t -> average pool -> its slice of `cat`; then the integral heads
static int run_resnet_towers_head(mpn_frcnn *p, const float *d_boxes, int N, int H, int W, hipStream_t s, int clamp) {
  const mpn_frcnn_config &c = p->cfg;
  int rc = mpn_foveal_forward(p->rois, N, p->fov, s);
  if (rc) return rc;
  const int Fcb = lin_np(c.fc_dim) / 8, Mp = lin_mp(N);
  // Two tower lanes (see mpn_frcnn::tower_stream): tower t on lane t & 1 — its own stream and activation buffers; the sorted / range-max
  // images of the feature map every tower pools from are built before the fork.  Tower t + 1's ROI pooling (a store-bound launch with no
  // matrix work), the ragged last block round and the launch gaps of each of a tower's ~20-80 convolutions then run under the other
  // lane's convolutions.  Pure scheduling: bit-identical results (the towers meet only in `cat`, each writing its own slice).
  // MEASURED (profiles/r06_tower_lanes_ab.txt): 10.86 -> 10.87 ms on configs[3] bf16, 23.61 -> 23.69 ms on configs[4] — nothing: two
  // towers' convolutions contend for the same vector-memory path that bounds each of them alone (the VGG towers' matrix-bound GEMMs are
  // a different story: 13.71 -> 13.43 ms, run_mpnet_head).  The graph lanes therefore exist in the debug flavour only (tower_lanes = 2).
  const bool lanes = p->tower_stream && resnet_has_second_lane(p->rn) && g_tower_lanes == 2 && p->rn_region.size() > 1 && !p->prof;
  if (lanes) {
    rc = resnet_heads_prepare(p->rn, s);
    if (rc) return rc;
    MPN_CHECK_HIP(hipEventRecord(p->ev_lane_go, s));
    MPN_CHECK_HIP(hipStreamWaitEvent(p->tower_stream, p->ev_lane_go, 0));
  }
  for (size_t t = 0; t < p->rn_region.size(); ++t) {
    const int ln = lanes ? (int)(t & 1) : 0;
    hipStream_t ls = ln ? p->tower_stream : s;
    SplitkSlotScope lane_slabs(ln ? SCR_GEMM_SPLITK_LANE : SCR_GEMM_SPLITK);  // (fp32 graphs: a pointwise layer of few tiles on the split-K GEMM)
    ProfScope ps(p, MPN_PROF_FC6, ls);
    rc = resnet_head_forward(p->rn, (int)t, p->fov + 5 * p->rn_region[t], 20, N, c.spatial_scale, p->cat + t * (size_t)Fcb * Mp * 8, Mp, ls, ln);
    if (rc) return rc;
  }
  if (lanes) {
    MPN_CHECK_HIP(hipEventRecord(p->ev_lane_done, p->tower_stream));
    MPN_CHECK_HIP(hipStreamWaitEvent(s, p->ev_lane_done, 0));
  }
  p->last_n = N;
  return run_integral_heads(p, d_boxes, N, H, W, (int)p->rn_region.size() - 1, s, clamp);
}

// The plain Fast R-CNN heads on fc7's output (VGG) / the pooled vector (ResNet, op-list), on stream hs: cls and bbox as one GEMM
// (model_utils.lua:105-119), softmax, decode (+ clamp).  `s`: the launch stream (hs != s: the side stream took the heads over).
static int run_plain_heads(mpn_frcnn *p, const float *y7, const float *dec_boxes, int N, int H, int W, hipStream_t hs, hipStream_t s, int clamp) {
  const mpn_frcnn_config &c = p->cfg;
  const int C = c.n_classes, F = c.fc_dim, K = p->n_integral, NH = plain_head_width(p);
  int rc;
  { ProfScope ps(p, MPN_PROF_HEADS, hs);
    SplitkSlotScope sk(hs != s ? SCR_GEMM_SPLITK_SIDE : SCR_GEMM_SPLITK);  // its partial sums must not share a buffer with fc6 / fc7 of the next image
    rc = linear_c8(y7, N, F, p->wh, p->bh, NH, 0, nullptr, p->head, hs, 0, nullptr, 1); }
  if (rc) return rc;
  ProfScope ps_post(p, MPN_PROF_POST, hs);
  // K integral classifiers (model_utils.lua:296-313): the mean of their softmaxes, read at the fused head's row pitch
  rc = K > 1 ? launch_integral_softmax_mean(p->head, NH, N, K, C, p->scores, hs) : launch_head_softmax(p->head, NH, N, C, p->scores, hs);
  if (rc) return rc;
  rc = launch_head_decode(p->head, NH, K * C, N, C, dec_boxes, c.bbox_mean, c.bbox_std, clamp, (float)W, (float)H, p->bbox_raw, p->bbox, hs);
  if (rc) return rc;
  p->last_n = N;
  return MPN_OK;
}

// resnet.lua:40-48: ROIPooling(14,14) -> layer4 -> average pool -> View; lands in y7 as the heads' operand
static int run_resnet_head(mpn_frcnn *p, const float *d_boxes, int N, int H, int W, hipStream_t s, int clamp) {
  p->y7_last = p->y7;
  int rc;
  { ProfScope ps(p, MPN_PROF_FC6, s); rc = resnet_head_forward(p->rn, 0, p->rois, 5, N, p->cfg.spatial_scale, p->y7, lin_mp(N), s); }
  return rc ? rc : run_plain_heads(p, p->y7, d_boxes, N, H, W, s, s, clamp);
}

// The VGG head's ROI pooling of the projected ROIs into fc6's operand, by one of four routes: from the pyramid's level stack or from
// the one map `feat` of record `m`, each from the pixel-major copy (built once per trunk run) or straight from the C8P map
static int vgg_roi_pool(mpn_frcnn *p, const Act &feat, mpn_frcnn::CachedMap *m, int N, hipStream_t s) {
  const mpn_frcnn_config &c = p->cfg;
  const RoiRule rule{1.0f, 0, c.roi_bin_rule};
  const bool pyr = p->n_scales > 1;
  int rc = MPN_OK;
  ProfScope ps(p, MPN_PROF_ROIPOOL, s);
  if (pyr && p->ms_pm && g_roi_pool_pm) {  // one pixel-major copy per computed level (once per image), the level read from column 0
    for (int l = 0; l < p->n_scales && !p->ms_pm_valid && rc == MPN_OK; ++l)
      if (p->ms_src[l] == l) rc = c8p_to_pixel_major(make_act(p->ms_feat + (size_t)l * p->ms_slot, feat.C, feat.H, feat.W), p->ms_pm + (size_t)l * p->ms_pm_slot, s);
    if (rc) return rc;
    p->ms_pm_valid = true;
    return roi_pool_pm(feat, p->ms_pm, p->rois, N, c.pooled_h, c.pooled_w, c.spatial_scale, rule, p->x6, s, 5, 0, LevelStack{p->ms_pm_slot, p->n_scales});
  }
  if (pyr) return roi_pool_c8(feat, p->rois, N, c.pooled_h, c.pooled_w, c.spatial_scale, rule, p->x6, nullptr, s, 5, 0, LevelStack{p->ms_slot, p->n_scales});
  if (m->pm && g_roi_pool_pm) {
    if (!m->pm_valid) { rc = c8p_to_pixel_major(feat, m->pm, s); if (rc) return rc; m->pm_valid = true; }  // once per trunk run
    return roi_pool_pm(feat, m->pm, p->rois, N, c.pooled_h, c.pooled_w, c.spatial_scale, rule, p->x6, s);
  }
  return roi_pool_c8(feat, p->rois, N, c.pooled_h, c.pooled_w, c.spatial_scale, rule, p->x6, nullptr, s);
}

// models/vgg.lua:23-31 behind the trunk: ROI pool -> fc6 -> fc7 -> heads.  The pipelined forms hand the heads over to the side stream
// after fc7 (mpn_frcnn::defer_stream): fc7 then writes buffer set defer_set's y7, and decode reads that set's copy of the boxes.
static int run_vgg_head(mpn_frcnn *p, const Act &feat, mpn_frcnn::CachedMap *m, const float *d_boxes, int N, int H, int W, hipStream_t s, int clamp) {
  const int F = p->cfg.fc_dim;
  hipStream_t hs = p->defer_stream ? p->defer_stream : s;
  float *y7 = hs != s ? p->y7_b[p->defer_set] : p->y7;
  p->y7_last = y7;
  const float *dec_boxes = d_boxes;
  int rc = vgg_roi_pool(p, feat, m, N, s);
  if (rc == MPN_OK) rc = fc_relu(p, MPN_PROF_FC6, p->x6, N, p->K6, p->w6, p->b6, p->w6_s3, p->x6_s3, p->y6, s, 0);
  if (rc == MPN_OK) rc = fc_relu(p, MPN_PROF_FC7, p->y6, N, F, p->w7, p->b7, p->w7_s3, p->y6_s3, y7, s, 0);
  if (rc) return rc;
  if (hs != s) {  // hand over: the side stream continues from here (its work on this buffer set is ordered by ev_tail[set])
    MPN_CHECK_HIP(hipEventRecord(p->ev_fc7, s));
    MPN_CHECK_HIP(hipStreamWaitEvent(hs, p->ev_fc7, 0));
    dec_boxes = p->boxes_b[p->defer_set];
#ifdef MPN_DEBUG_HOOKS
    if (g_defer_heads == 2) hipLaunchKernelGGL(side_stream_delay_kernel, dim3(1), dim3(64), 0, hs, 100000ll);
#endif
  }
  return run_plain_heads(p, y7, dec_boxes, N, H, W, hs, s, clamp);
}

// One ImageDetect:detect (ImageDetect.lua:100-193) on record `m` (see obtain_features): getImages' size, the features, the ROI
// projection, then the head of the handle's kind.
static int run_detect(mpn_frcnn *p, const float *d_image, int H0, int W0, const float *d_boxes, int N, hipStream_t s, int clamp, mpn_frcnn::CachedMap *m) {
  const mpn_frcnn_config &c = p->cfg;
  MPN_CHECK_ARG(p && d_boxes);
  p->seg_shape[0][0] = -1;  // SEG_HEAD: the host-side state a captured head graph relies on is being rewritten (run_segment re-stamps it after its body)
  MPN_CHECK_ARG(H0 > 0 && W0 > 0 && N > 0 && N <= c.max_rois);
  double sc = 1.0;  // scale_target == 0 keeps the image as it is (s = 1)
  int H = H0, W = W0;
  const bool pyr = p->n_scales > 1;  // an image pyramid (mpn_frcnn_set_scales): its levels' sizes are run_pyramid_trunk's
  if (!pyr && c.scale_target > 0.0) sc = getimages_size(H0, W0, c.scale_target, c.scale_max, &H, &W);
  if (H <= 0 || W <= 0 || (!pyr && (H > c.max_h || W > c.max_w))) {
    set_error("run_detect: %dx%d image (scaled to %dx%d) exceeds the pipeline's %dx%d", H0, W0, H, W, c.max_h, c.max_w);
    return MPN_EINVAL;
  }
  Act feat;
  int rc = obtain_features(p, d_image, H0, W0, H, W, sc, m, s, &feat);
  if (rc) return rc;
  const bool vgg = !p->rn && !p->is_mpnet;
  rc = pyr ? project_im_rois_levels(d_boxes, N, p->n_scales, p->ms_scales, p->rois, s)
           : (vgg && p->defer_stream) ? project_im_rois_copy(d_boxes, N, sc, p->rois, p->boxes_b[p->defer_set], s) : mpn_project_im_rois(d_boxes, N, sc, p->rois, s);
  if (rc) return rc;
  // decode uses the ORIGINAL boxes and clamps to the ORIGINAL image (ImageDetect.lua:183-185, Tester_FRCNN.lua:75-78)
  if (p->is_mpnet) { p->last_n = N; return run_mpnet_head(p, feat, d_boxes, N, H0, W0, s, clamp); }
  if (p->rn) return p->rn_region.empty() ? run_resnet_head(p, d_boxes, N, H0, W0, s, clamp) : run_resnet_towers_head(p, d_boxes, N, H0, W0, s, clamp);
  return run_vgg_head(p, feat, m, d_boxes, N, H0, W0, s, clamp);
}

// Horizontal-flip test-time augmentation around run_detect (include/mpn.h mpn_frcnn_set_augment): the upright
// half unclamped with its tables kept aside, the mirrored half (the ORIGINAL image mirrored in front of getImages, flipBoxes of the
// boxes) unclamped, then one merge launch that leaves the merged tables where every later stage reads them (p->scores / p->bbox).
// Plain Fast R-CNN handles keep both final maps cached, so d_image == nullptr runs both heads on them; the other handle kinds run
// two whole passes through the one (upright) record and keep the mirrored map only.  All of it is stream work on library-owned buffers: it captures into a head graph.
static int run_detect_aug(mpn_frcnn *p, const float *d_image, int H0, int W0, const float *d_boxes, int N, hipStream_t s, int clamp) {
  if (!p->augment) return run_detect(p, d_image, H0, W0, d_boxes, N, s, clamp, &p->up);
  const int C = p->cfg.n_classes;
  const bool two_maps = p->mir.buf != nullptr;
  if (!d_image && !two_maps) {
    set_error("run_detect: augmentation on a %s handle keeps one trunk map, so a detect on cached features has no upright map to read: pass the image",
              handle_kind_name(p));
    return MPN_EINVAL;
  }
  MPN_CHECK_ARG(d_boxes && H0 > 0 && W0 > 0 && N > 0 && N <= p->cfg.max_rois);
  int rc = d_image ? p->own.grow(&p->aug_img, &p->aug_img_bytes, (size_t)3 * H0 * W0 * sizeof(float), s) : MPN_OK;
  if (rc) return rc;
  rc = run_detect(p, d_image, H0, W0, d_boxes, N, s, 0, &p->up);
  if (rc) return rc;
  MPN_CHECK_HIP(hipMemcpyAsync(p->aug_scores, p->scores, (size_t)N * C * sizeof(float), hipMemcpyDeviceToDevice, s));
  MPN_CHECK_HIP(hipMemcpyAsync(p->aug_bbox, p->bbox, (size_t)N * 4 * C * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (d_image) {
    ProfScope ps(p, MPN_PROF_TRANSFORM, s);
    rc = mpn_image_hflip(d_image, 3, H0, W0, p->aug_img, s);
    if (rc) return rc;
  }
  rc = mpn_flip_boxes(d_boxes, N, W0, p->aug_boxes, s);
  if (rc) return rc;
  rc = run_detect(p, d_image ? p->aug_img : nullptr, H0, W0, p->aug_boxes, N, s, 0, two_maps ? &p->mir : &p->up);
  if (rc) return rc;
  ProfScope ps(p, MPN_PROF_POST, s);
  return launch_augment_merge(p->aug_scores, p->aug_bbox, p->scores, p->bbox, N, C, clamp, (float)W0, (float)H0, s);
}

extern "C" int mpn_frcnn_detect(mpn_frcnn *p, const float *d_image, int H, int W, const float *d_boxes, int N,
                                float *d_scores, float *d_bbox, int clamp, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  ScratchScope scratch_scope(&p->scratch);
  { int rcf = mpn_frcnn_flush(p, stream); if (rcf) return rcf; }  // a pipelined predecessor's side-stream work may still use the head buffers
  hipStream_t s = as_stream(stream);
  int rc = run_detect_aug(p, d_image, H, W, d_boxes, N, s, clamp ? 1 : 0);
  if (rc) return rc;
  const int C = p->cfg.n_classes;
  if (d_scores) MPN_CHECK_HIP(hipMemcpyAsync(d_scores, p->scores, (size_t)N * C * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (d_bbox) MPN_CHECK_HIP(hipMemcpyAsync(d_bbox, p->bbox, (size_t)N * 4 * C * sizeof(float), hipMemcpyDeviceToDevice, s));
  return MPN_OK;
}

static void select_set(mpn_frcnn *p, int b) {
  p->scored = p->scored_b[b]; p->keep = p->keep_b[b]; p->keep_idx = p->keep_idx_b[b];
  p->counts = p->counts_b[b]; p->n_keep = p->n_keep_b[b]; p->thresh = p->thresh_b[b];
  p->voted = p->voted_b[b];
}

// ---- captured launch graphs (see mpn_frcnn::GraphKey) --------------------------------------------------------------------------
enum { SEG_HEAD = 0, SEG_TAIL = 1, SEG_SHARD_NMS = 2, SEG_SHARD_FIN = 3 };
constexpr size_t kMaxGraphs = 64;  // per handle: a caller that passes fresh pointers on every call must not grow the cache without bound

// Runs body(stream) — a pure chain of stream work plus host-side bookkeeping — for segment `kind`, or replays its captured graph.
// stable_ptrs: the key's pointers are library-owned (staging sets): capture at the first sighting; caller-provided pointers are captured
// at their second sighting (a caller that hands in fresh buffers every call never pays for a capture).
template <class F>
static int run_segment(mpn_frcnn *p, int kind, const mpn_frcnn::GraphKey &key, const int (&shape)[4], bool stable_ptrs, hipStream_t s, F &&body) {
  int *last = p->seg_shape[kind];
  const bool same_shape = memcmp(last, shape, sizeof(shape)) == 0;
  auto direct = [&]() -> int {
    const int rc = body(s);
    memcpy(last, shape, sizeof(shape));
    if (rc) last[0] = -2;  // a failed run leaves no state to rely on
    return rc;
  };
  if (!p->graphs_on || p->prof) return direct();
  auto it = p->graphs.find(key);
  int seen_before = 0;
  if (it == p->graphs.end()) {
    if (!stable_ptrs) {  // first sighting of caller-provided pointers: remember the key in the side ring only
      int hit = -1;
      for (int q = 0; q < mpn_frcnn::kUnseen; ++q) {
        const mpn_frcnn::GraphKey &u = p->unseen[kind][q];
        if (p->unseen_valid[kind][q] && !(u < key) && !(key < u)) { hit = q; break; }
      }
      if (hit < 0) {
        const int q = p->unseen_next[kind];
        p->unseen[kind][q] = key; p->unseen_valid[kind][q] = true;
        p->unseen_next[kind] = (q + 1) % mpn_frcnn::kUnseen;
        return direct();
      }
      p->unseen_valid[kind][hit] = false;
      seen_before = 1;
    }
    if (p->graphs.size() >= kMaxGraphs) {  // full: drop the entries that hold no executable graph (failed / never captured) before giving up
      for (auto j = p->graphs.begin(); j != p->graphs.end();) j = j->second.exec ? std::next(j) : p->graphs.erase(j);
      if (p->graphs.size() >= kMaxGraphs) {  // all live: evict the least recently used one
        auto lru = p->graphs.begin();
        for (auto j = p->graphs.begin(); j != p->graphs.end(); ++j) if (j->second.last_use < lru->second.last_use) lru = j;
        // its last replay may still be in flight (the pipelined forms put no bound on how far the host runs ahead): wait for the stream it
        // was launched on before the executable goes away.  Evictions are rare — a host must rotate > 64 live keys to get here.
        if (lru->second.launched) (void)hipStreamSynchronize(lru->second.last_stream);
        (void)hipGraphExecDestroy(lru->second.exec);
        p->graphs.erase(lru);
      }
    }
    it = p->graphs.emplace(key, mpn_frcnn::GraphEntry()).first;
    it->second.seen = seen_before;
  }
  mpn_frcnn::GraphEntry &e = it->second;
  e.last_use = ++p->graph_clock;
  if (e.exec && e.gen != alloc_generation()) {  // a library buffer was replaced since (the regrow synchronised its stream; a replay on another stream may still run)
    if (e.launched && e.last_stream != s) (void)hipStreamSynchronize(e.last_stream);
    (void)hipGraphExecDestroy(e.exec); e.exec = nullptr;
  }
  if (e.exec && same_shape) {
    MPN_CHECK_HIP(hipGraphLaunch(e.exec, s));
    e.last_stream = s; e.launched = true;
    ++p->graph_replays;
    return MPN_OK;
  }
  ++e.seen;
  if (!same_shape || e.failed || (!stable_ptrs && e.seen < 2)) return direct();  // the warm-up run for this shape / this key
  if (!p->cap_stream && p->own.stream(&p->cap_stream) != MPN_OK) { (void)hipGetLastError(); e.failed = true; return direct(); }
  if (hipStreamBeginCapture(p->cap_stream, hipStreamCaptureModeRelaxed) != hipSuccess) { (void)hipGetLastError(); e.failed = true; return direct(); }
  const int rc_body = body(p->cap_stream);  // host bookkeeping happens, the stream work is recorded instead of executed
  hipGraph_t g = nullptr;
  const hipError_t ec = hipStreamEndCapture(p->cap_stream, &g);
  hipGraphExec_t ex = nullptr;
  if (rc_body == MPN_OK && ec == hipSuccess && g && hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) == hipSuccess && ex) {
    (void)hipGraphDestroy(g);
    e.exec = ex; e.gen = alloc_generation();
    ++p->graph_captures;
    memcpy(last, shape, sizeof(shape));
    MPN_CHECK_HIP(hipGraphLaunch(e.exec, s));
    e.last_stream = s; e.launched = true;
    return MPN_OK;
  }
  if (g) (void)hipGraphDestroy(g);
  (void)hipGetLastError();
  e.failed = true;     // this chain cannot be captured here: never try again, run it as ordinary launches
  return direct();
}

// Tester_FRCNN.lua:111-124 for the classes [c0, c1) (0-based, background left out) of the current buffer set: per-class NMS of the
// selected boxes (`rows` per class at most), then bbox voting if configured.  under_trunk: the pipelined tail's NMS form (mpn_internal.h)
static int nms_and_vote(mpn_frcnn *p, int c0, int c1, int rows, hipStream_t q, bool under_trunk) {
  const mpn_frcnn_config &c = p->cfg;
  const size_t off = (size_t)c0 * rows;
  int r;
  { ProfScope ps(p, MPN_PROF_NMS, q);
    r = under_trunk ? nms_batched_under_trunk(p->scored + off * 5, p->counts + c0, c1 - c0, rows, c.nms_thresh, p->keep + off * 5, p->keep_idx + off, p->n_keep + c0, q)
                    : mpn_nms_batched(p->scored + off * 5, p->counts + c0, c1 - c0, rows, c.nms_thresh, p->keep + off * 5, p->keep_idx + off, p->n_keep + c0, q); }
  if (r || !c.bbox_voting) return r;
  return mpn_bbox_vote_batched(p->keep + off * 5, p->n_keep + c0, p->scored + off * 5, p->counts + c0, c1 - c0, rows, c.bbox_vote_thresh,
                               c.bbox_vote_score_pow != 0.0f ? c.bbox_vote_score_pow : 1.0f, p->voted + off * 5, q);
}

// Tester_FRCNN.lua:106-125 + keep_top_k: per class j=1..C-1 select (score > thresh) -> NMS -> top-k, on stream `t`
static int run_tail(mpn_frcnn *p, int N, float *d_dets, int top_cap, int *d_n_dets, hipStream_t sel_stream, hipStream_t t,
                    hipEvent_t after_select) {
  const mpn_frcnn_config &c = p->cfg;
  const int C = c.n_classes;
  int rc;
  float *sc, *bb;
  joined_tables(p, &sc, &bb);
  { ProfScope ps(p, MPN_PROF_SELECT, sel_stream);
    rc = mpn_select_scored(sc, bb, N, C, 1, c.score_thresh, p->scored, p->counts, nullptr, sel_stream); }
  if (rc) return rc;
  if (after_select) {  // hand over to the side stream
    MPN_CHECK_HIP(hipEventRecord(after_select, sel_stream));
    MPN_CHECK_HIP(hipStreamWaitEvent(t, after_select, 0));
  }
  const mpn_frcnn::GraphKey key{SEG_TAIL, d_dets, d_n_dets, p->scored, nullptr, N, top_cap, 0, 0};  // p->scored names the buffer set
  const int shape[4] = {N, top_cap, c.bbox_voting ? 1 : 0, 0};
  return run_segment(p, SEG_TAIL, key, shape, false, t, [&](hipStream_t q) -> int {
    const int r = nms_and_vote(p, 0, C - 1, N, q, after_select != nullptr);
    if (r) return r;
    ProfScope ps(p, MPN_PROF_TOPK, q);
    return mpn_keep_top_k_sorted(c.bbox_voting ? p->voted : p->keep, p->n_keep, C - 1, N, c.top_k, p->thresh, d_dets, top_cap, d_n_dets, q);  // NMS / voted tables: scores non-increasing per class
  });
}

// Tester_FRCNN.lua:72-100: detect (clamped, :75-78); for i = 2..num_iter: SelectBoxes on the previous pass -> detect on the refined
// boxes with recompute_features = false (NOT clamped: only the first bbox_pred is); the rows of all passes are concatenated
// before the per-class NMS.  opt.test_use_rbox_scores (:91-97): the scores of pass i+1 go with the boxes of pass i.
static int run_detect_iter(mpn_frcnn *p, const float *d_image, int H, int W, const float *d_boxes, int N, hipStream_t s, int *n_rows) {
  int rc = run_detect_aug(p, d_image, H, W, d_boxes, N, s, 1);
  *n_rows = N;
  const mpn_frcnn_config &c = p->cfg;
  if (rc || c.num_iter <= 1) return rc;
  const int C = c.n_classes;
  const size_t srow = (size_t)N * C, brow = (size_t)N * 4 * C;
  const bool rbox = c.use_rbox_scores != 0;
  for (int it = 1;; ++it) {  // pass `it` (1-based) has just run: p->scores / p->bbox hold its output
    const int sslot = rbox ? it - 2 : it - 1, bslot = it - 1;  // rbox: drop the first score table and the last box table
    if (sslot >= 0) MPN_CHECK_HIP(hipMemcpyAsync(p->it_scores + sslot * srow, p->scores, srow * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (!(rbox && it == c.num_iter)) MPN_CHECK_HIP(hipMemcpyAsync(p->it_bbox + bslot * brow, p->bbox, brow * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (it == c.num_iter) break;
    rc = mpn_select_boxes_forward(p->scores, p->bbox, N, C, p->it_boxes, s);
    if (rc) return rc;
    rc = run_detect_aug(p, nullptr, H, W, p->it_boxes, N, s, 0);
    if (rc) return rc;
  }
  *n_rows = n_passes(c) * N;
  return MPN_OK;
}

// the head segment: run_detect_iter as a captured graph when it starts from an image (the cached-features form keeps host-side
// checks of what is cached and always runs as ordinary launches)
static int run_head(mpn_frcnn *p, const float *d_image, int H, int W, const float *d_boxes, int N, hipStream_t s, int *n_rows, bool stable_ptrs) {
  if (!d_image || !d_boxes || N <= 0 || N > p->cfg.max_rois) {
    const int rc = run_detect_iter(p, d_image, H, W, d_boxes, N, s, n_rows);
    p->seg_shape[SEG_HEAD][0] = -1;
    return rc;
  }
  *n_rows = n_passes(p->cfg) * N;
  const mpn_frcnn::GraphKey key{SEG_HEAD, d_image, d_boxes, nullptr, nullptr, H, W, N, 0};
  const int shape[4] = {H, W, N, 1};
  const int rc = run_segment(p, SEG_HEAD, key, shape, stable_ptrs, s, [&](hipStream_t q) -> int {
    int rows = 0;
    return run_detect_iter(p, d_image, H, W, d_boxes, N, q, &rows);
  });
  if (rc == MPN_OK) p->last_n = N;  // (a replay runs no host code)
  return rc;
}

static int join_tail(mpn_frcnn *p, int b, hipStream_t s) {
  if (p->tail_pending[b]) {
    MPN_CHECK_HIP(hipStreamWaitEvent(s, p->ev_tail[b], 0));
    p->tail_pending[b] = false;
  }
  return MPN_OK;
}

extern "C" int mpn_frcnn_flush(mpn_frcnn *p, void *stream) {
  MPN_CHECK_ARG(p != nullptr);
  hipStream_t s = as_stream(stream);
  int rc = join_tail(p, 0, s);
  if (rc) return rc;
  return join_tail(p, 1, s);
}

extern "C" int mpn_frcnn_test_one(mpn_frcnn *p, const float *d_image, int H, int W, const float *d_boxes, int N,
                                  float *d_dets, int top_cap, int *d_n_dets, void *stream) {
  MPN_CHECK_ARG(p != nullptr && d_n_dets && (top_cap == 0 || d_dets) && top_cap >= 0);
  ScratchScope scratch_scope(&p->scratch);
  hipStream_t s = as_stream(stream);
  int rc = mpn_frcnn_flush(p, stream);  // a pipelined predecessor may still own a buffer set
  if (rc) return rc;
  int rows = N;
  rc = run_head(p, d_image, H, W, d_boxes, N, s, &rows, false);
  if (rc) return rc;
  select_set(p, 0);
  p->last_rows = rows;
  return run_tail(p, rows, d_dets, top_cap, d_n_dets, s, s, nullptr);
}

// ------------------------------------------------------------------------------------------------------------------------------
// Proposal (ROI) sharding of ONE image across the GPUs of a node — the latency mode of SURVEY §8e / north_star's
// "images+proposals shard across the 8 GPUs".  Replaces ModelParallelTable.lua:195-242 (broadcast the whole input to every tower
// GPU, run the towers, copy their outputs back and concatenate): here every rank runs the trunk on the image (1.6 ms of replicated
// work instead of a 5-62 MB feature broadcast over xGMI), the ROI head on ITS rows of the proposal table, the per-class NMS on
// ITS classes; what travels is scored boxes only — one all-gather of the decoded rows ([N/G, 5C] per rank: 420 KB in total for
// VOC, 1.6 MB for COCO) and one of the kept tables.  Rows are independent (ImageDetect.lua:126-133's chunk invariance) and
// classes are independent (Tester_FRCNN.lua:106-125's loop), so the result is the unsharded mpn_frcnn_test_one's bit for bit.
// The three steps take caller-provided records so that the exchange between them can be any transport; mpn_frcnn_test_one_sharded
// chains them over an mpn_comm (RCCL all-gather, comm.hip).
static int refuse_multi_pass(const mpn_frcnn *p, const char *form);
// the sharded forms cut the head by class into records of 5C floats per row: a plain handle with K > 1 integral classifiers has no such layout
static int refuse_shard_integral(const mpn_frcnn *p, const char *form) {
  if (!plain_integral(p)) return MPN_OK;
  set_error("%s: not supported on a handle with %d integral classifiers (mpn_frcnn_create_integral): the sharded records hold one classifier; use mpn_frcnn_test_one", form, p->n_integral);
  return MPN_ESTATE;
}

extern "C" int mpn_shard_range(int n, int world, int rank, int *lo, int *hi) {
  MPN_CHECK_ARG(n >= 0 && world >= 1 && rank >= 0 && rank < world && lo && hi);
  shard_bounds(n, world, rank, lo, hi);
  return MPN_OK;
}

extern "C" size_t mpn_frcnn_shard_rows_floats(const mpn_frcnn *p, int N, int world) {
  if (!p || N <= 0 || world < 1) return 0;
  const int chunk = (N + world - 1) / world;
  return (size_t)n_passes(p->cfg) * chunk * 5 * p->cfg.n_classes;
}

extern "C" size_t mpn_frcnn_shard_class_floats(const mpn_frcnn *p, int N, int world) {
  if (!p || N <= 0 || world < 1) return 0;
  const int n_cls = p->cfg.n_classes - 1, cmax = (n_cls + world - 1) / world;
  return shard_class_rec_floats(cmax, n_passes(p->cfg) * N, p->cfg.bbox_voting);
}

extern "C" int mpn_frcnn_shard_head(mpn_frcnn *p, const float *d_image, int H, int W, const float *d_boxes, int N, int rank, int world,
                                    float *d_rows_rec, void *stream) {
  MPN_CHECK_ARG(p != nullptr && d_boxes && d_rows_rec && N > 0 && N <= p->cfg.max_rois && world >= 1 && rank >= 0 && rank < world);
  if (int ri = refuse_shard_integral(p, "mpn_frcnn_shard_head")) return ri;
  if (int rp = refuse_multi_pass(p, "mpn_frcnn_shard_head")) return rp;
  ScratchScope scratch_scope(&p->scratch);
  hipStream_t s = as_stream(stream);
  int rc = mpn_frcnn_flush(p, stream);
  if (rc) return rc;
  const mpn_frcnn_config &c = p->cfg;
  const int C = c.n_classes, P = n_passes(c), chunk = (N + world - 1) / world;
  int lo, hi;
  shard_bounds(N, world, rank, &lo, &hi);
  const int n_local = hi - lo;
  const size_t total = (size_t)P * chunk * 5 * C;
  if (n_local == 0) {  // more ranks than proposals: nothing to score here
    MPN_CHECK_HIP(hipMemsetAsync(d_rows_rec, 0, total * sizeof(float), s));
    return MPN_OK;
  }
  int rows = n_local;
  rc = run_head(p, d_image, H, W, d_boxes + 4 * (size_t)lo, n_local, s, &rows, false);
  if (rc) return rc;
  float *sc, *bb;
  joined_tables(p, &sc, &bb);
  hipLaunchKernelGGL(shard_pack_rows_kernel, dim3((unsigned)cdiv_sz(total, 256)), dim3(256), 0, s, sc, bb, n_local, P, C, chunk, d_rows_rec);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

extern "C" int mpn_frcnn_shard_nms(mpn_frcnn *p, const float *d_rows_all, int N, int rank, int world, float *d_class_rec, void *stream) {
  MPN_CHECK_ARG(p != nullptr && d_rows_all && d_class_rec && N > 0 && N <= p->cfg.max_rois && world >= 1 && rank >= 0 && rank < world);
  if (int ri = refuse_shard_integral(p, "mpn_frcnn_shard_nms")) return ri;
  ScratchScope scratch_scope(&p->scratch);
  hipStream_t s = as_stream(stream);
  int rc = mpn_frcnn_flush(p, stream);
  if (rc) return rc;
  const mpn_frcnn_config &c = p->cfg;
  const int C = c.n_classes, P = n_passes(c), chunk = (N + world - 1) / world, rows = P * N;
  // the whole image's joined tables, in the unsharded row order, where run_tail reads them
  float *sc, *bb;
  joined_tables(p, &sc, &bb);
  const size_t rec_floats = (size_t)P * chunk * 5 * C, total = (size_t)rows * 5 * C;
  select_set(p, 0);
  p->last_rows = rows;
  p->last_n = N;
  const int n_cls = C - 1, cmax = (n_cls + world - 1) / world;
  int c0, c1;
  shard_bounds(n_cls, world, rank, &c0, &c1);
  const mpn_frcnn::GraphKey key{SEG_SHARD_NMS, d_rows_all, d_class_rec, nullptr, nullptr, N, rank, world, 0};
  const int shape[4] = {N, rank, world, c.bbox_voting ? 1 : 0};
  return run_segment(p, SEG_SHARD_NMS, key, shape, false, s, [&](hipStream_t q) -> int {
    hipLaunchKernelGGL(shard_unpack_rows_kernel, dim3((unsigned)cdiv_sz(total, 256)), dim3(256), 0, q, d_rows_all, N, world, P, C, chunk, rec_floats, sc, bb);
    MPN_CHECK_LAUNCH();
    int r;
    { ProfScope ps(p, MPN_PROF_SELECT, q);
      r = mpn_select_scored(sc, bb, rows, C, 1, c.score_thresh, p->scored, p->counts, nullptr, q); }
    if (r) return r;
    if (c1 > c0 && (r = nms_and_vote(p, c0, c1, rows, q, false)) != MPN_OK) return r;
    hipLaunchKernelGGL(shard_pack_classes_kernel, dim3(cdiv(rows, 256), cmax), dim3(256), 0, q, p->keep, p->keep_idx, p->n_keep,
                       c.bbox_voting ? p->voted : nullptr, c0, c1, rows, cmax, d_class_rec);
    MPN_CHECK_LAUNCH();
    return MPN_OK;
  });
}

extern "C" int mpn_frcnn_shard_finish(mpn_frcnn *p, const float *d_class_all, int N, int world, float *d_dets, int top_cap, int *d_n_dets,
                                      void *stream) {
  MPN_CHECK_ARG(p != nullptr && d_class_all && N > 0 && N <= p->cfg.max_rois && world >= 1);
  MPN_CHECK_ARG(d_n_dets && (top_cap == 0 || d_dets) && top_cap >= 0);
  if (int ri = refuse_shard_integral(p, "mpn_frcnn_shard_finish")) return ri;
  ScratchScope scratch_scope(&p->scratch);
  hipStream_t s = as_stream(stream);
  const mpn_frcnn_config &c = p->cfg;
  const int n_cls = c.n_classes - 1, cmax = (n_cls + world - 1) / world, rows = n_passes(c) * N;
  select_set(p, 0);
  p->last_rows = rows;
  const mpn_frcnn::GraphKey key{SEG_SHARD_FIN, d_class_all, d_dets, d_n_dets, nullptr, N, world, top_cap, 0};
  const int shape[4] = {N, world, top_cap, c.bbox_voting ? 1 : 0};
  return run_segment(p, SEG_SHARD_FIN, key, shape, false, s, [&](hipStream_t q) -> int {
    hipLaunchKernelGGL(shard_unpack_classes_kernel, dim3(cdiv(rows, 256), n_cls), dim3(256), 0, q, d_class_all, n_cls, world, rows, cmax,
                       shard_class_rec_floats(cmax, rows, c.bbox_voting), p->keep, p->keep_idx, p->n_keep, c.bbox_voting ? p->voted : nullptr);
    MPN_CHECK_LAUNCH();
    ProfScope ps(p, MPN_PROF_TOPK, q);
    return mpn_keep_top_k_sorted(c.bbox_voting ? p->voted : p->keep, p->n_keep, n_cls, rows, c.top_k, p->thresh, d_dets, top_cap, d_n_dets, q);
  });
}

extern "C" int mpn_frcnn_test_one_sharded(mpn_frcnn *p, mpn_comm *comm, const float *d_image, int H, int W, const float *d_boxes, int N,
                                          float *d_dets, int top_cap, int *d_n_dets, void *stream) {
  MPN_CHECK_ARG(p != nullptr && comm != nullptr && N > 0);
  if (int ri = refuse_shard_integral(p, "mpn_frcnn_test_one_sharded")) return ri;
  if (int rp = refuse_multi_pass(p, "mpn_frcnn_test_one_sharded")) return rp;
  hipStream_t s = as_stream(stream);
  const int world = mpn_comm_world(comm), rank = mpn_comm_rank(comm);
  MPN_CHECK_ARG(world >= 1 && rank >= 0);
  const size_t rr = mpn_frcnn_shard_rows_floats(p, N, world), cr = mpn_frcnn_shard_class_floats(p, N, world);
  const size_t floats[4] = {rr, rr * world, cr, cr * world};
  int rc;
  for (int i = 0; i < 4; ++i)
    if ((rc = p->own.grow(&p->sh_buf[i], &p->sh_bytes[i], floats[i] * sizeof(float), s)) != MPN_OK) return rc;
  rc = mpn_frcnn_shard_head(p, d_image, H, W, d_boxes, N, rank, world, p->sh_buf[0], stream);
  if (rc) return rc;
  rc = mpn_gather_rows(comm, p->sh_buf[0], rr, p->sh_buf[1], stream);
  if (rc) return rc;
  rc = mpn_frcnn_shard_nms(p, p->sh_buf[1], N, rank, world, p->sh_buf[2], stream);
  if (rc) return rc;
  rc = mpn_gather_rows(comm, p->sh_buf[2], cr, p->sh_buf[3], stream);
  if (rc) return rc;
  return mpn_frcnn_shard_finish(p, p->sh_buf[3], N, world, d_dets, top_cap, d_n_dets, stream);
}

// Throughput form for a loop over images (Tester:test, Tester_FRCNN.lua:150-157): trunk + heads + select of
// image i on `stream`; NMS + top-k of image i on the pipeline's side stream, overlapping image
// i+1's MFMA kernels (they are latency-bound on ~20 CUs).  d_dets / d_n_dets of call i are ordered on `stream`
// only after call i+1 returns or after mpn_frcnn_flush(); the caller alternates two output buffers.
// the throughput and sharded forms run one trunk pass per image only: single-scale (include/mpn.h mpn_frcnn_set_scales), no flip
// augmentation (mpn_frcnn_set_augment)
static int refuse_multi_pass(const mpn_frcnn *p, const char *form) {
  if (p->augment) {
    set_error("%s: not supported with horizontal-flip augmentation (mpn_frcnn_set_augment): use mpn_frcnn_test_one", form);
    return MPN_EINVAL;
  }
  if (p->n_scales <= 1) return MPN_OK;
  set_error("%s: not supported with an image pyramid (mpn_frcnn_set_scales, %d scales): use mpn_frcnn_test_one", form, p->n_scales);
  return MPN_EINVAL;
}

static int pipelined_impl(mpn_frcnn *p, const float *d_image, int H, int W, const float *d_boxes, int N, float *d_dets, int top_cap, int *d_n_dets,
                          void *stream, bool stable_ptrs) {
  MPN_CHECK_ARG(p != nullptr && d_n_dets && (top_cap == 0 || d_dets) && top_cap >= 0);
  if (int rp = refuse_multi_pass(p, "mpn_frcnn_test_one_pipelined")) return rp;
  ScratchScope scratch_scope(&p->scratch);
  hipStream_t s = as_stream(stream);
  const int b = (int)(p->seq & 1);
  int rc = join_tail(p, b, s);  // buffer set b was last used two calls ago
  if (rc) return rc;
  int rows = N;
  // heads + softmax + decode + select on the side stream too (plain VGG head, one localisation pass, no captured graphs, not profiling)
  const bool defer = g_defer_heads && !p->is_mpnet && !p->rn && p->cfg.num_iter == 1 && !p->graphs_on && !p->prof && d_image && d_boxes;
  if (defer) {
    if (!p->ev_fc7) {  // first use.  All or nothing, as in mpn_frcnn_set_augment: ev_fc7 comes last, its presence says that all of them exist
      p->y7_b[0] = p->y7;
      int rca = p->own.alloc(&p->y7_b[1], (size_t)(lin_np(p->cfg.fc_dim) / 8) * p->Mp * 8 * sizeof(float), true);
      for (int i = 0; i < 2 && !rca; ++i) rca = p->own.alloc(&p->boxes_b[i], (size_t)p->cfg.max_rois * 4 * sizeof(float));
      if (!rca) rca = p->own.event(&p->ev_fc7);
      if (rca) {  // the next call starts from scratch
        for (float **q : {&p->y7_b[1], &p->boxes_b[0], &p->boxes_b[1]}) p->own.free_now(q);
        return rca;
      }
    }
    p->defer_stream = p->side; p->defer_set = b;
  } else if (p->was_deferred) {  // the form changed under us (graphs / profiling switched on): the side stream may still read y7_b[0] == y7
    rc = mpn_frcnn_flush(p, stream);
    if (rc) return rc;
  }
  p->was_deferred = defer;
  rc = run_head(p, d_image, H, W, d_boxes, N, s, &rows, stable_ptrs);
  p->defer_stream = nullptr;
  if (rc) return rc;
  select_set(p, b);
  p->last_rows = rows;
  rc = run_tail(p, rows, d_dets, top_cap, d_n_dets, defer ? p->side : s, p->side, p->ev_head[b]);
  if (rc) return rc;
  MPN_CHECK_HIP(hipEventRecord(p->ev_tail[b], p->side));
  p->tail_pending[b] = true;
  rc = join_tail(p, b ^ 1, s);  // the previous image's detections become visible to `stream` here
  p->seq++;
  return rc;
}

extern "C" int mpn_frcnn_test_one_pipelined(mpn_frcnn *p, const float *d_image, int H, int W, const float *d_boxes, int N,
                                            float *d_dets, int top_cap, int *d_n_dets, void *stream) {
  return pipelined_impl(p, d_image, H, W, d_boxes, N, d_dets, top_cap, d_n_dets, stream, false);
}

// Host-fed throughput form: the reference's loop hands testOne a CPU image and CPU boxes (Tester_FRCNN.lua:64-66) and
// ImageDetect copies them to the GPU (ImageDetect.lua:148-151).  Here the upload of image i is issued on the handle's copy
// stream into staging set i & 1 — it runs while image i-1's kernels are still executing — and `stream` waits for it only
// at the point where the trunk starts.  The copy stream in turn waits until image i-2 (the previous user of the set) has
// been consumed.
extern "C" int mpn_frcnn_test_one_pipelined_host(mpn_frcnn *p, const float *h_image, int H, int W, const float *h_boxes, int N,
                                                 float *d_dets, int top_cap, int *d_n_dets, void *stream) {
  MPN_CHECK_ARG(p != nullptr && h_image && h_boxes && H > 0 && W > 0 && N > 0 && N <= p->cfg.max_rois);
  if (int rp = refuse_multi_pass(p, "mpn_frcnn_test_one_pipelined_host")) return rp;
  hipStream_t s = as_stream(stream);
  const size_t img_bytes = (size_t)3 * H * W * sizeof(float);
  if (!p->copy) {  // first use: events, the box staging buffers, the copy stream.  All or nothing, as in mpn_frcnn_set_augment: the stream
    int rc0 = MPN_OK;  // comes last, its presence says that all of them exist
    for (int i = 0; i < mpn_frcnn::kStage && !rc0; ++i) {
      rc0 = p->own.event(&p->ev_up[i]);
      if (!rc0) rc0 = p->own.event(&p->ev_consumed[i]);
      if (!rc0) rc0 = p->own.alloc(&p->stage_boxes[i], (size_t)p->cfg.max_rois * 4 * sizeof(float));
    }
    if (!rc0) rc0 = p->own.stream(&p->copy);
    if (rc0) {  // the next call starts from scratch
      for (int i = 0; i < mpn_frcnn::kStage; ++i) { p->own.drop(&p->ev_up[i]); p->own.drop(&p->ev_consumed[i]); p->own.free_now(&p->stage_boxes[i]); }
      return rc0;
    }
  }
  const int b = (int)(p->up_seq % mpn_frcnn::kStage);
  if (img_bytes > p->stage_bytes[b]) {  // image staging grows on demand (getImages may be handed images larger than max_h x max_w)
    MPN_CHECK_HIP(hipStreamSynchronize(p->copy));  // the set's last upload (grow_device_buffer waits for `s`)
    const int rcg = p->own.grow(&p->stage_img[b], &p->stage_bytes[b], std::max(img_bytes, (size_t)3 * p->cfg.max_h * p->cfg.max_w * sizeof(float)), s);
    if (rcg) return rcg;
  }
  // The staging set is free once the image that used it (three calls ago) has been consumed.  Waited for on the HOST, not with
  // hipStreamWaitEvent on the copy stream: a copy that depends on a compute-queue event leaves the SDMA path (measured on AlexNet,
  // tools/host_enqueue_probe.py: 0.99 ms / image with the stream wait, 0.86 resident), and this bounds the host's run-ahead to
  // three images, as a queue should.
  if (p->used_pending[b]) { MPN_CHECK_HIP(hipEventSynchronize(p->ev_consumed[b])); p->used_pending[b] = false; }
  MPN_CHECK_HIP(hipMemcpyAsync(p->stage_img[b], h_image, img_bytes, hipMemcpyHostToDevice, p->copy));
  // (Round 5 tried the proposal table's copy on the launch stream instead — small copies are shader blits, i.e. a kernel on the copy stream's
  // hardware queue — and took it back: a 32-KB table there stalls the launch stream for 0.25 ms per image, 5.40 -> 5.65 ms at 2000 proposals.)
  MPN_CHECK_HIP(hipMemcpyAsync(p->stage_boxes[b], h_boxes, (size_t)N * 4 * sizeof(float), hipMemcpyHostToDevice, p->copy));
  MPN_CHECK_HIP(hipEventRecord(p->ev_up[b], p->copy));
  MPN_CHECK_HIP(hipStreamWaitEvent(s, p->ev_up[b], 0));
  int rc = pipelined_impl(p, p->stage_img[b], H, W, p->stage_boxes[b], N, d_dets, top_cap, d_n_dets, stream, true);  // staging sets: stable pointers
  if (rc) return rc;
  // the image is consumed by the trunk's first kernel and the boxes by the decode kernel: both are behind this point of `stream`
  MPN_CHECK_HIP(hipEventRecord(p->ev_consumed[b], s));
  p->used_pending[b] = true;
  p->up_seq++;
  return MPN_OK;
}

extern "C" int mpn_frcnn_create(const mpn_frcnn_config *cfg, const float *const *d_conv_w, const float *const *d_conv_b,
                                const float *d_fc6_w, const float *d_fc6_b, const float *d_fc7_w, const float *d_fc7_b,
                                const float *d_cls_w, const float *d_cls_b, const float *d_bbox_w, const float *d_bbox_b,
                                mpn_frcnn **out) {
  return mpn_frcnn_create_integral(cfg, d_conv_w, d_conv_b, d_fc6_w, d_fc6_b, d_fc7_w, d_fc7_b, d_cls_w, d_cls_b, d_bbox_w, d_bbox_b, 1, out);
}

extern "C" int mpn_frcnn_create_integral(const mpn_frcnn_config *cfg, const float *const *d_conv_w, const float *const *d_conv_b,
                                         const float *d_fc6_w, const float *d_fc6_b, const float *d_fc7_w, const float *d_fc7_b,
                                         const float *d_cls_w, const float *d_cls_b, const float *d_bbox_w, const float *d_bbox_b,
                                         int n_integral, mpn_frcnn **out) {
  return create_handle(CreateArgs{cfg, d_conv_w, d_conv_b, d_fc6_w, d_fc6_b, d_fc7_w, d_fc7_b, d_cls_w, d_cls_b, d_bbox_w, d_bbox_b, nullptr, nullptr, nullptr,
                                  n_integral}, out);
}

extern "C" int mpn_frcnn_n_integral(const mpn_frcnn *p) { return p ? p->n_integral : 0; }

extern "C" int mpn_mpnet_create(const mpn_frcnn_config *cfg, const float *const *d_conv_w, const float *const *d_conv_b,
                                const mpn_mpnet_weights *mw, const float *d_cls_w, const float *d_cls_b,
                                const float *d_bbox_w, const float *d_bbox_b, mpn_frcnn **out) {
  MPN_CHECK_ARG(mw != nullptr);
  return create_handle(CreateArgs{cfg, d_conv_w, d_conv_b, nullptr, nullptr, nullptr, nullptr, d_cls_w, d_cls_b, d_bbox_w, d_bbox_b, mw, nullptr, nullptr}, out);
}

extern "C" int mpn_resnet_create(const mpn_frcnn_config *cfg, const mpn_resnet_weights *rw, const float *d_cls_w, const float *d_cls_b,
                                 const float *d_bbox_w, const float *d_bbox_b, mpn_frcnn **out) {
  MPN_CHECK_ARG(rw != nullptr);
  return create_handle(CreateArgs{cfg, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, d_cls_w, d_cls_b, d_bbox_w, d_bbox_b, nullptr, rw, nullptr}, out);
}

extern "C" int mpn_graph_create(const mpn_frcnn_config *cfg, const mpn_graph_weights *gw, const float *d_cls_w, const float *d_cls_b,
                                const float *d_bbox_w, const float *d_bbox_b, mpn_frcnn **out) {
  MPN_CHECK_ARG(gw != nullptr);
  return create_handle(CreateArgs{cfg, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, d_cls_w, d_cls_b, d_bbox_w, d_bbox_b, nullptr, nullptr, gw}, out);
}

extern "C" int mpn_frcnn_set_graphs(mpn_frcnn *p, int enable) {
  MPN_CHECK_ARG(p != nullptr);
  p->graphs_on = enable ? 1 : 0;
  return MPN_OK;
}

// a setter that changes what a detect computes: every captured launch graph and every cached trunk map of the handle goes
static int drop_graphs_and_features(mpn_frcnn *p) {
  MPN_CHECK_HIP(hipDeviceSynchronize());  // no replay or cached map of the old setting may still be in flight
  for (auto &kv : p->graphs) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
  p->graphs.clear();
  for (int k = 0; k < 4; ++k) {
    p->unseen_next[k] = 0;
    for (int q = 0; q < mpn_frcnn::kUnseen; ++q) p->unseen_valid[k][q] = false;
    for (int j = 0; j < 4; ++j) p->seg_shape[k][j] = -1;
  }
  p->up.invalidate();  // cached trunk outputs: gone (the next detect must pass an image)
  p->mir.invalidate();
  p->ms_h0 = p->ms_w0 = -1;
  return MPN_OK;
}

extern "C" int mpn_frcnn_set_scales(mpn_frcnn *p, int n_scales, const double *h_targets) {
  if (n_scales < 0 || n_scales > MPN_MAX_SCALES || (n_scales > 0 && !h_targets)) {
    set_error("mpn_frcnn_set_scales: n_scales %d outside 0..MPN_MAX_SCALES (%d) or no targets", n_scales, MPN_MAX_SCALES);
    return MPN_EINVAL;
  }
  for (int l = 0; l < n_scales; ++l)
    if (!(std::isfinite(h_targets[l]) && h_targets[l] > 0.0)) { set_error("mpn_frcnn_set_scales: target %d is %g (must be finite and > 0)", l, h_targets[l]); return MPN_EINVAL; }
  MPN_CHECK_ARG(p != nullptr);
  if (n_scales > 1 && (p->is_mpnet || p->rn)) {
    set_error("mpn_frcnn_set_scales: a %s handle has no image pyramid (only mpn_frcnn_create's VGG Fast R-CNN head pools from one)",
              handle_kind_name(p));
    return MPN_EINVAL;
  }
  if (n_scales > 1 && p->augment) {
    set_error("mpn_frcnn_set_scales: an image pyramid (%d scales) and horizontal-flip augmentation exclude each other: call mpn_frcnn_set_augment(p, 0) first", n_scales);
    return MPN_EINVAL;
  }
  int rc_drop = drop_graphs_and_features(p);
  if (rc_drop) return rc_drop;
  if (n_scales <= 1) {
    p->n_scales = 0;
    p->cfg.scale_target = n_scales == 1 ? h_targets[0] : p->create_scale_target;
    return MPN_OK;
  }
  if (n_scales > p->ms_cap) {  // per-level slots at the largest canvas geometry
    int fh = p->cfg.max_h, fw = p->cfg.max_w;
    final_map_size(p, &fh, &fw);
    const size_t slot = act_bytes(p->feat_c, fh, fw) / sizeof(float), pm_slot = pixel_major_elems(make_act(nullptr, p->feat_c, fh, fw));
    bump_alloc_generation();  // (behind drop_graphs_and_features' device synchronise; both buffers go, then both come back cleared)
    p->own.free_now(&p->ms_feat);
    p->own.free_now(&p->ms_pm);
    p->ms_cap = 0; p->n_scales = 0;
    int rc = p->own.alloc_slot(&p->ms_feat, slot * n_scales * sizeof(float), true);
    if (!rc) rc = p->own.alloc_slot(&p->ms_pm, pm_slot * n_scales * sizeof(float), true);
    if (rc) return rc;
    p->ms_slot = slot; p->ms_pm_slot = pm_slot; p->ms_cap = n_scales;
  }
  p->n_scales = n_scales;
  for (int l = 0; l < n_scales; ++l) p->scale_targets[l] = h_targets[l];
  return MPN_OK;
}

extern "C" int mpn_frcnn_set_augment(mpn_frcnn *p, int enable) {
  MPN_CHECK_ARG(p != nullptr);
  const bool plain = !p->is_mpnet && !p->rn;
  if (enable && p->n_scales > 1) {
    set_error("mpn_frcnn_set_augment: horizontal-flip augmentation and an image pyramid (mpn_frcnn_set_scales, %d scales) exclude each other: "
              "restore a single scale first", p->n_scales);
    return MPN_EINVAL;
  }
  if (enable && !plain && p->cfg.num_iter > 1) {
    set_error("mpn_frcnn_set_augment: a %s handle keeps one trunk map, and iterative localisation (num_iter %d) under augmentation needs the "
              "upright and the mirrored one cached (only mpn_frcnn_create handles hold both): create the handle with num_iter 1", handle_kind_name(p), p->cfg.num_iter);
    return MPN_EINVAL;
  }
  int rc = drop_graphs_and_features(p);
  if (rc) return rc;
  if (p->rn) resnet_drop_features(p->rn);
  p->augment = 0;
  if (!enable) return MPN_OK;
  if (!p->aug_scores) {  // first use: the second half's buffers, sized for max_rois rows and the max_h x max_w geometry
    const size_t M = (size_t)p->cfg.max_rois, C = (size_t)p->cfg.n_classes;
    const size_t img_bytes = (size_t)3 * p->cfg.max_h * p->cfg.max_w * sizeof(float);
    bump_alloc_generation();
    for (float **q : {&p->aug_img, &p->aug_boxes, &p->aug_bbox, &p->mir.buf, &p->mir.pm}) p->own.free_now(q);  // (an earlier attempt that ran out of memory)
    p->aug_img_bytes = 0;
    if ((rc = p->own.alloc_slot(&p->aug_img, img_bytes))) return rc;
    p->aug_img_bytes = img_bytes;
    if ((rc = p->own.alloc_slot(&p->aug_boxes, M * 4 * sizeof(float)))) return rc;
    if ((rc = p->own.alloc_slot(&p->aug_bbox, M * 4 * C * sizeof(float)))) return rc;
    if (plain) {
      int fh = p->cfg.max_h, fw = p->cfg.max_w;
      final_map_size(p, &fh, &fw);
      const size_t feat_bytes = act_bytes(p->feat_c, fh, fw), pm_bytes = pixel_major_elems(make_act(nullptr, p->feat_c, fh, fw)) * sizeof(float);
      if ((rc = p->own.alloc_slot(&p->mir.buf, feat_bytes, true))) return rc;
      if ((rc = p->own.alloc_slot(&p->mir.pm, pm_bytes, true))) return rc;
    }
    if ((rc = p->own.alloc_slot(&p->aug_scores, M * C * sizeof(float)))) return rc;  // last: its presence says that all of them exist
  }
  p->augment = 1;
  return MPN_OK;
}

extern "C" int mpn_frcnn_graph_stats(const mpn_frcnn *p, long *captures, long *replays) {
  MPN_CHECK_ARG(p != nullptr);
  if (captures) *captures = p->graph_captures;
  if (replays) *replays = p->graph_replays;
  return MPN_OK;
}

extern "C" int mpn_frcnn_set_profiling(mpn_frcnn *p, int enable) {
  MPN_CHECK_ARG(p != nullptr);
  p->prof = enable != 0;
  return MPN_OK;
}

extern "C" int mpn_frcnn_get_profile(mpn_frcnn *p, double *ms, long *counts, int n_tags, int reset) {
  MPN_CHECK_ARG(p != nullptr && ms && counts && n_tags >= MPN_PROF_NTAGS);
  MPN_CHECK_HIP(hipDeviceSynchronize());
  for (size_t i = 0; i + 1 < p->ev_used + 1 && i / 2 < p->ev_tag.size(); i += 2) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, p->ev_pool[i], p->ev_pool[i + 1]) == hipSuccess) {
      p->prof_ms[p->ev_tag[i / 2]] += t;
      p->prof_cnt[p->ev_tag[i / 2]] += 1;
    }
  }
  p->ev_used = 0;
  p->ev_tag.clear();
  for (int t = 0; t < MPN_PROF_NTAGS; ++t) { ms[t] = p->prof_ms[t]; counts[t] = p->prof_cnt[t]; }
  if (reset) for (int t = 0; t < MPN_PROF_NTAGS; ++t) { p->prof_ms[t] = 0; p->prof_cnt[t] = 0; }
  return MPN_OK;
}

extern "C" int mpn_frcnn_nms_results(mpn_frcnn *p, const float **d_keep, const int **d_keep_idx, const int **d_n_keep,
                                     int *m_stride) {
  MPN_CHECK_ARG(p != nullptr);
  MPN_CHECK_HIP(hipDeviceSynchronize());
  if (d_keep) *d_keep = (p->cfg.bbox_voting && p->voted) ? p->voted : p->keep;  // what testOne returns as img_boxes[j]
  if (d_keep_idx) *d_keep_idx = p->keep_idx;
  if (d_n_keep) *d_n_keep = p->n_keep;
  if (m_stride) *m_stride = p->last_rows ? p->last_rows : p->last_n;
  return MPN_OK;
}

// Training (mpn_frcnn_train_*, mpn_frcnn_get_head_weights / _get_trunk_weights and their debug hooks) is a translation unit of its own:
// train_driver.hip, over pipeline.h.  This file meets it in mpn_frcnn_destroy and mpn_frcnn_debug_tensor alone.

#ifdef MPN_DEBUG_HOOKS
// bench.py's `power_sensitivity` leg (debug flavour only): fc6 of the VGG Fast R-CNN pipeline issued `iters` times BACK TO BACK on the
// operand the last detect() left in HBM (the ROI-pooled, post-ReLU conv5 features and the handle's own fc6 weights) — the same GEMM that
// mpn_debug_bench_linear times on dense random operands.  Inside the pipeline fc6 follows the trunk's phases and runs at a higher clock.
extern "C" int mpn_debug_bench_fc6(mpn_frcnn *p, int iters, float *ms_out) {
  MPN_CHECK_ARG(p && iters > 0 && ms_out);
  if (p->rn || p->is_mpnet || p->last_n <= 0) { set_error("mpn_debug_bench_fc6: needs a VGG Fast R-CNN handle after a detect()"); return MPN_ESTATE; }
  ScratchScope scratch_scope(&p->scratch);
  const int N = p->last_n, F = p->cfg.fc_dim;
  return time_back_to_back(iters, ms_out, [&] { return linear_c8(p->x6, N, p->K6, p->w6, p->b6, F, 1, p->y6, nullptr, nullptr, 0, nullptr, 1); });
}
// tests/test_gpu_box_kernels_numerics.py (debug flavour only): ONE of the four score / box kernels between the last GEMM and NMS, through the
// pipeline's own launcher, on caller-supplied device buffers.  `which`: 0 head_softmax_kernel (d_a = head [M, ld], d_out = scores [M, C]);
// 1 integral_softmax_mean_kernel (d_a = logits [M, K*C], d_out = scores [M, C]); 2 head_decode_kernel (d_a = head [M, ld], deltas at columns
// col0 .. col0 + 4C, d_b = boxes [M, 4], h_mean4 / h_std4 = the BBoxNorm constants or both NULL for none, d_raw [M, 4C] or NULL, d_out = boxes
// [M, 4C]); 3 augment_merge_kernel (d_a = upright scores [M, C], d_b = upright boxes [M, 4C], d_raw = the mirrored half's scores and d_out its
// boxes, both merged in place).  Refuses what handle creation refuses for the pipeline (C < 1, C > 256 for the integral kernel, M < 0); M == 0
// launches nothing.
extern "C" int mpn_debug_head_post(int which, const float *d_a, const float *d_b, int ld, int col0, int M, int C, int K, const float *h_mean4,
                                   const float *h_std4, int clamp, float im_w, float im_h, float *d_raw, float *d_out, void *stream) {
  MPN_CHECK_ARG(which >= 0 && which <= 3 && M >= 0 && C >= 1);
  hipStream_t s = as_stream(stream);
  static const float zero4[4] = {0.f, 0.f, 0.f, 0.f};
  switch (which) {
    case 0:
      MPN_CHECK_ARG(ld >= C);
      if (M == 0) return MPN_OK;
      MPN_CHECK_ARG(d_a && d_out);
      return launch_head_softmax(d_a, ld, M, C, d_out, s);
    case 1:
      MPN_CHECK_ARG(C <= 256 && K >= 1);
      if (M == 0) return MPN_OK;
      MPN_CHECK_ARG(d_a && d_out);
      return launch_integral_softmax_mean(d_a, K * C, M, K, C, d_out, s);
    case 2:
      MPN_CHECK_ARG(col0 >= 0 && ld >= col0 + 4 * C && (h_mean4 != nullptr) == (h_std4 != nullptr));
      if (M == 0) return MPN_OK;
      MPN_CHECK_ARG(d_a && d_b && d_out);
      return launch_head_decode(d_a, ld, col0, M, C, d_b, h_mean4 ? h_mean4 : zero4, h_std4 ? h_std4 : zero4, clamp, im_w, im_h, d_raw, d_out, s);
    default:
      if (M == 0) return MPN_OK;
      MPN_CHECK_ARG(d_a && d_b && d_raw && d_out);
      return launch_augment_merge(d_a, d_b, d_raw, d_out, M, C, clamp, im_w, im_h, s);
  }
}
#endif

// the debug tensor's buffer (the caller has synchronised the device).  Not DeviceOwner::grow: no kernel of a captured graph reads dbg, and
// a generation bump here would cost the caller its graphs
int mpn::grow_dbg(mpn_frcnn *p, size_t bytes) {
  if (bytes <= p->dbg_bytes) return MPN_OK;
  p->own.free_now(&p->dbg);
  const int rc = p->own.alloc_slot(&p->dbg, bytes);
  p->dbg_bytes = rc == MPN_OK ? bytes : 0;
  return rc;
}

extern "C" int mpn_frcnn_debug_tensor(mpn_frcnn *p, const char *name, const float **d_ptr, size_t *n_elems) {
  MPN_CHECK_ARG(p && name && d_ptr && n_elems);
  if (!strncmp(name, "train_", 6)) {  // the training state's tensors (train_driver.hip)
    bool known = false;
    const int rct = train_debug_tensor(p, name, d_ptr, n_elems, &known);
    if (known) return rct;
  }
  if (!strncmp(name, "tower_train_", 12)) return tower_train_debug_tensor(p, name, d_ptr, n_elems);
  if (plain_integral(p) && !strcmp(name, "cls")) {
    set_error("mpn_frcnn_debug_tensor: invalid argument: a handle with %d integral classifiers keeps no single 'cls': ask for \"cls_k\" ([N, K * C])", p->n_integral);
    return MPN_EINVAL;
  }
  if (p->last_n <= 0 || (!p->rn && p->last_h <= 0)) { set_error("mpn_frcnn_debug_tensor: run detect first"); return MPN_ESTATE; }
  const mpn_frcnn_config &c = p->cfg;
  const int N = p->last_n, C = c.n_classes, F = c.fc_dim, PP = c.pooled_h * c.pooled_w;
  int h = p->last_h, w = p->last_w;
  final_map_size(p, &h, &w);
  std::string nm(name);
  size_t n = 0;
  int level = -1;  // "conv5.<l>": level l of the image pyramid
  if (nm.compare(0, 6, "conv5.") == 0 && nm.size() == 7 && nm[6] >= '0' && nm[6] < '0' + MPN_MAX_SCALES) {
    level = nm[6] - '0';
    if (p->n_scales <= 1 || level >= p->n_scales) { set_error("mpn_frcnn_debug_tensor: '%s' needs an image pyramid of more than %d levels", name, level); return MPN_EINVAL; }
    if (p->ms_h0 < 0) { set_error("mpn_frcnn_debug_tensor: no pyramid maps cached (run detect with an image first)"); return MPN_ESTATE; }
    n = (size_t)p->feat_c * h * w;
  } else if (nm == "conv5") n = (size_t)p->feat_c * h * w;
  else if (nm == "rois") n = (size_t)N * 5;
  else if (nm == "pooled") n = (size_t)N * p->feat_c * PP;
  else if (nm == "fc7") n = (size_t)N * F;
  else if (nm == "cls") n = (size_t)N * C;
  else if (nm == "bbox_raw") n = (size_t)N * 4 * C;
  else if (nm == "cls_k") n = (size_t)N * p->n_integral * C;                       // integral heads: the K classifiers' logits [N, K * C] (pre-softmax)
  else if (nm == "cat") n = (size_t)N * (p->is_mpnet ? p->towers.size() : p->rn_region.size()) * F;  // tower outputs side by side [N, towers * F]
  else { set_error("mpn_frcnn_debug_tensor: unknown tensor '%s'", name); return MPN_EINVAL; }
  const bool towers = p->is_mpnet || (p->rn && !p->rn_region.empty());
  if ((nm == "cls_k" || nm == "cat") && (!towers || lin_np(F) != F) && !(nm == "cls_k" && plain_integral(p))) { set_error("mpn_frcnn_debug_tensor: '%s' needs a tower model (integral heads)", name); return MPN_EINVAL; }
  if (p->is_mpnet && nm != "conv5" && nm != "bbox_raw" && nm != "cls_k" && nm != "cat") { set_error("mpn_frcnn_debug_tensor: '%s' is not kept by the MultiPathNet head", name); return MPN_EINVAL; }
  if (p->rn && nm != "bbox_raw" && nm != "cls_k" && nm != "cat" && !((nm == "cls" || nm == "fc7") && p->rn_region.empty())) { set_error("mpn_frcnn_debug_tensor: '%s' is not kept by the op-list / ResNet pipelines", name); return MPN_EINVAL; }
  MPN_CHECK_HIP(hipDeviceSynchronize());
  if (int rcd = grow_dbg(p, n * sizeof(float))) return rcd;
  int rc = MPN_OK;
  if (level >= 0 || (nm == "conv5" && p->n_scales > 1)) {
    const int l = p->ms_src[level >= 0 ? level : 0];
    rc = c8p_to_nchw(make_act(p->ms_feat + (size_t)l * p->ms_slot, p->feat_c, h, w), p->dbg, nullptr);
  } else if (nm == "conv5") {
    const ConvLayer &L = p->conv.back();
    rc = c8p_to_nchw(make_act(L.pool ? L.pooled : L.out, p->feat_c, h, w), p->dbg, nullptr);
  } else if (nm == "rois") {
    MPN_CHECK_HIP(hipMemcpy(p->dbg, p->rois, n * sizeof(float), hipMemcpyDeviceToDevice));
  } else if (nm == "pooled") {
    rc = launch_unpack_pooled(p->x6, N, p->feat_c, PP, lin_mp(N), p->dbg);
  } else if (nm == "fc7") {
    rc = c8_to_rowmajor(p->y7_last ? p->y7_last : p->y7, N, F, p->dbg, nullptr);  // rows at stride lin_mp(N), as linear_c8 wrote them
  } else if (nm == "cls_k" && plain_integral(p)) {  // the first K * C columns of the fused head
    hipLaunchKernelGGL(copy_cols_kernel, dim3((unsigned)cdiv_sz(n, 256)), dim3(256), 0, nullptr, p->head, plain_head_width(p), 0, N, p->n_integral * C, p->dbg);
    MPN_CHECK_LAUNCH();
  } else if (nm == "cls_k") {
    MPN_CHECK_HIP(hipMemcpy(p->dbg, p->cls_rm, n * sizeof(float), hipMemcpyDeviceToDevice));
  } else if (nm == "cat") {
    rc = c8_to_rowmajor(p->cat, N, (int)(n / N), p->dbg, nullptr);  // towers' [F/8][Mp][8] blocks back to back == one C8 matrix of towers * F columns
  } else if (nm == "cls") {
    hipLaunchKernelGGL(copy_cols_kernel, dim3((unsigned)cdiv_sz(n, 256)), dim3(256), 0, nullptr, p->head, plain_head_width(p), 0, N, C, p->dbg);
    MPN_CHECK_LAUNCH();
  } else {
    MPN_CHECK_HIP(hipMemcpy(p->dbg, p->bbox_raw, n * sizeof(float), hipMemcpyDeviceToDevice));
  }
  if (rc) return rc;
  MPN_CHECK_HIP(hipDeviceSynchronize());
  *d_ptr = p->dbg;
  *n_elems = n;
  return MPN_OK;
}

#ifdef MPN_DEBUG_HOOKS
// tests/test_gpu_layout_kernels.py: this file's glue kernels one launch at a time, with the grids their call
// sites above use, on the null stream.  Rules: layout_debug.h.
#include "layout_debug.h"

// dst [M, ncols] = columns [col0, col0 + ncols) of src [M, ld]
extern "C" int mpn_debug_copy_cols(const float *d_src, size_t src_bytes, int ld, int col0, int M, int ncols, float *d_dst, size_t dst_bytes) {
  MPN_CHECK_ARG(M > 0 && ncols > 0 && col0 >= 0 && ld >= col0 + ncols);
  LDBG_BUF(d_src, src_bytes, ((size_t)(M - 1) * ld + col0 + ncols) * sizeof(float), 4);
  LDBG_BUF(d_dst, dst_bytes, (size_t)M * ncols * sizeof(float), 4);
  const size_t n = (size_t)M * ncols;
  hipLaunchKernelGGL(copy_cols_kernel, dim3((unsigned)cdiv_sz(n, 256)), dim3(256), 0, nullptr, d_src, ld, col0, M, ncols, d_dst);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// rank `rank` of `world`: its tables sc [P * n_local, C], bb [P * n_local, 4C] (n_local from shard_bounds; null when it is 0) -> its
// row record [P * chunk * 5C], chunk = ceil(N / world) as mpn_frcnn_shard_head computes it
extern "C" int mpn_debug_shard_pack_rows(const float *d_sc, size_t sc_bytes, const float *d_bb, size_t bb_bytes, int N, int world, int rank, int P, int C,
                                         float *d_rec, size_t rec_bytes) {
  MPN_CHECK_ARG(N > 0 && world >= 1 && rank >= 0 && rank < world && P > 0 && C > 0);
  const int chunk = (N + world - 1) / world;
  int lo, hi;
  shard_bounds(N, world, rank, &lo, &hi);
  const int n_local = hi - lo;
  if (n_local > 0) {
    LDBG_BUF(d_sc, sc_bytes, (size_t)P * n_local * C * sizeof(float), 4);
    LDBG_BUF(d_bb, bb_bytes, (size_t)P * n_local * 4 * C * sizeof(float), 4);
  }
  const size_t total = (size_t)P * chunk * 5 * C;
  LDBG_BUF(d_rec, rec_bytes, total * sizeof(float), 4);
  hipLaunchKernelGGL(shard_pack_rows_kernel, dim3((unsigned)cdiv_sz(total, 256)), dim3(256), 0, nullptr, d_sc, d_bb, n_local, P, C, chunk, d_rec);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// all ranks' row records [world][P * chunk * 5C] -> sc [P * N, C], bb [P * N, 4C]
extern "C" int mpn_debug_shard_unpack_rows(const float *d_all, size_t all_bytes, int N, int world, int P, int C, float *d_sc, size_t sc_bytes, float *d_bb,
                                           size_t bb_bytes) {
  MPN_CHECK_ARG(N > 0 && world >= 1 && P > 0 && C > 0);
  const int chunk = (N + world - 1) / world;
  const size_t rec_floats = (size_t)P * chunk * 5 * C, total = (size_t)P * N * 5 * C;
  LDBG_BUF(d_all, all_bytes, (size_t)world * rec_floats * sizeof(float), 4);
  LDBG_BUF(d_sc, sc_bytes, (size_t)P * N * C * sizeof(float), 4);
  LDBG_BUF(d_bb, bb_bytes, (size_t)P * N * 4 * C * sizeof(float), 4);
  hipLaunchKernelGGL(shard_unpack_rows_kernel, dim3((unsigned)cdiv_sz(total, 256)), dim3(256), 0, nullptr, d_all, N, world, P, C, chunk, rec_floats, d_sc, d_bb);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// keep / voted [n_cls, rows, 5], kidx [n_cls, rows], n_keep [n_cls] -> the class record of `rank` (shard_class_rec_floats); d_voted null: no voting
extern "C" int mpn_debug_shard_pack_classes(const float *d_keep, size_t keep_bytes, const int *d_kidx, size_t kidx_bytes, const int *d_n_keep,
                                            size_t n_keep_bytes, const float *d_voted, size_t voted_bytes, int n_cls, int world, int rank, int rows,
                                            float *d_rec, size_t rec_bytes) {
  MPN_CHECK_ARG(n_cls > 0 && world >= 1 && rank >= 0 && rank < world && rows > 0 && n_cls <= 65535);
  const int cmax = (n_cls + world - 1) / world;
  int c0, c1;
  shard_bounds(n_cls, world, rank, &c0, &c1);
  LDBG_BUF(d_keep, keep_bytes, (size_t)n_cls * rows * 5 * sizeof(float), 4);
  LDBG_BUF(d_kidx, kidx_bytes, (size_t)n_cls * rows * sizeof(int), 4);
  LDBG_BUF(d_n_keep, n_keep_bytes, (size_t)n_cls * sizeof(int), 4);
  if (d_voted) LDBG_BUF(d_voted, voted_bytes, (size_t)n_cls * rows * 5 * sizeof(float), 4);
  LDBG_BUF(d_rec, rec_bytes, shard_class_rec_floats(cmax, rows, d_voted != nullptr) * sizeof(float), 4);
  hipLaunchKernelGGL(shard_pack_classes_kernel, dim3(cdiv(rows, 256), cmax), dim3(256), 0, nullptr, d_keep, d_kidx, d_n_keep, d_voted, c0, c1, rows, cmax, d_rec);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// all ranks' class records -> the per-class tables
extern "C" int mpn_debug_shard_unpack_classes(const float *d_all, size_t all_bytes, int n_cls, int world, int rows, float *d_keep, size_t keep_bytes,
                                              int *d_kidx, size_t kidx_bytes, int *d_n_keep, size_t n_keep_bytes, float *d_voted, size_t voted_bytes) {
  MPN_CHECK_ARG(n_cls > 0 && world >= 1 && rows > 0 && n_cls <= 65535);
  const int cmax = (n_cls + world - 1) / world;
  const size_t rec_floats = shard_class_rec_floats(cmax, rows, d_voted != nullptr);
  LDBG_BUF(d_all, all_bytes, (size_t)world * rec_floats * sizeof(float), 4);
  LDBG_BUF(d_keep, keep_bytes, (size_t)n_cls * rows * 5 * sizeof(float), 4);
  LDBG_BUF(d_kidx, kidx_bytes, (size_t)n_cls * rows * sizeof(int), 4);
  LDBG_BUF(d_n_keep, n_keep_bytes, (size_t)n_cls * sizeof(int), 4);
  if (d_voted) LDBG_BUF(d_voted, voted_bytes, (size_t)n_cls * rows * 5 * sizeof(float), 4);
  hipLaunchKernelGGL(shard_unpack_classes_kernel, dim3(cdiv(rows, 256), n_cls), dim3(256), 0, nullptr, d_all, n_cls, world, rows, cmax, rec_floats, d_keep,
                     d_kidx, d_n_keep, d_voted);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}
#endif
