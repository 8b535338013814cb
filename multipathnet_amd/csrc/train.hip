// train.hip — training the Fast R-CNN head on the device with the trunk frozen (train.lua:154-158, BBoxRegressionCriterion.lua,
// BatchProviderROI.lua:125-131, engines/Optim.lua).  gfx950 only.
//
// A step is deterministic: without dropout (the reference's opt.train_remove_dropouts = true) and with it (its default; dropout_c8 below,
// whose mask is a counter-based function of seed, step, layer, row and column).
//
// The three Linear layers behind the ROI pooling keep their weights in the packed MFMA order [K64/8][NP][8] that the forward GEMM
// reads (dense.h), and training updates them IN PLACE in that order.  The contraction of a weight gradient runs over the B ~ 128 ROI
// rows only, so the fc6 update (411 MB of weights at VGG-16) is a streaming kernel: per step it reads and writes the weights and their
// momentum once, and the gradient tile lives in MFMA accumulators between the two — it never reaches memory.
//
// One operand mapping serves both matrix kernels.  Both MFMA operands are "records": 8 consecutive floats of a C8 matrix row or of a
// packed weight row, one 32-byte load per lane.  With v_mfma_f32_32x32x2_f32 (D[i][j] += A[i][kk] B[kk][j], lane l holds A[l % 32][l / 32]
// and B[l / 32][l % 32]) lane l loads the record of K CHUNK ck0 + l % 32 at contraction index 2 s + l / 32 and issues EIGHT MFMAs, one per
// float e of the record: accumulator e then holds D_e[i][j] for k = (ck0 + i) * 8 + e.  A lane owns D_e[8 (r / 4) + 4 (l / 32) + r % 4][l % 32]
// in register r, so for a fixed r its eight accumulators are the 8 floats of ONE record of the result — chunk ck0 + i, column l % 32 —
// and the 32 lanes of a half-wave store 1 KiB contiguous.
#include "train.h"

#include <algorithm>
#include <cstdint>

#include "dense.h"
#include "philox.h"

namespace mpn {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------------------------
// Loss + gradient w.r.t. the head's output
// ---------------------------------------------------------------------------------------------------------------------------------
// K classifiers in the row (the integral loss, model_utils.lua:275-317), of which classifier k is trained: its logits are columns
// [c0, c0 + C), c0 = k * C; the box outputs start at column cb = K * C.  K = 1, k = 0 is the plain head (c0 = 0, cb = C).
// SPLIT (the tower models' head: two GEMMs, two outputs): the logits are rows of `cls` [B, K * C], the box outputs rows of `box` [B, 4C],
// and the gradient goes to two C8 matrices, g [ceil(KC/8)][Mp][8] and g_box [ceil(4C/8)][Mp][8] — K * C is in general no multiple of 8,
// so the fused matrix cannot be cut by a pointer.  Otherwise cls = the fused row, box = cls + K * C, one matrix g over all (K+4)C columns.
template <bool SPLIT>
__global__ __launch_bounds__(256) void train_loss_kernel(const float *__restrict__ cls, int ld_cls, const float *__restrict__ box, int ld_box, int B, int C,
                                                         int K, int k, const float *__restrict__ rois, const float *__restrict__ gt,
                                                         const int *__restrict__ labels, LossCfg cfg, float *__restrict__ g, float *__restrict__ g_box,
                                                         int Mp, float *__restrict__ loss) {
  __shared__ float s_cls[256], s_box[256];
  const int c0 = k * C, cb = K * C;
  const float invB = 1.0f / (float)B, gbox = cfg.bbox_weight / (float)B;
  float acc_cls = 0.0f, acc_box = 0.0f;
  for (int i = threadIdx.x; i < B; i += 256) {  // one row per thread, rows ascending
    const float *z = cls + (size_t)i * ld_cls + c0, *tb = box + (size_t)i * ld_box;  // the selected classifier's logits; the row's box outputs
    int y = labels[i];
    y = y < 0 ? 0 : (y >= C ? C - 1 : y);
    float mx = z[0];
    for (int c = 1; c < C; ++c) mx = z[c] > mx ? z[c] : mx;
    float sum = 0.0f;
    for (int c = 0; c < C; ++c) sum += expf(z[c] - mx);
    acc_cls += (mx + logf(sum)) - z[y];  // log-sum-exp: finite for any finite logits
    float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (y > 0) {  // utils.convertTo(roi, gt), then BatchProviderROI.lua:125-131's normalisation
      const float *r = rois + (size_t)i * 4, *t = gt + (size_t)i * 4;
      const float xc = (r[0] + r[2]) * 0.5f, yc = (r[1] + r[3]) * 0.5f, w = r[2] - r[0], h = r[3] - r[1];
      const float xtc = (t[0] + t[2]) * 0.5f, ytc = (t[1] + t[3]) * 0.5f, wt = t[2] - t[0], ht = t[3] - t[1];
      float tg[4] = {(xtc - xc) / w, (ytc - yc) / h, logf(wt / w), logf(ht / h)};
      float row = 0.0f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (cfg.norm) tg[j] = (tg[j] - cfg.mean[j]) / cfg.std[j];
        d[j] = tb[4 * y + j] - tg[j];
        const float a = fabsf(d[j]);
        row += a < 1.0f ? 0.5f * d[j] * d[j] : a - 0.5f;
      }
      acc_box += row;
    }
    const float inv_sum = 1.0f / sum;
    // column n of the K classifiers' block / of the box block: every other classifier's columns, every other class's four: exactly +0.0
    auto cls_val = [&](int n) -> float {
      return (n >= c0 && n < c0 + C) ? (expf(z[n - c0] - mx) * inv_sum - (n - c0 == y ? 1.0f : 0.0f)) * invB : 0.0f;
    };
    auto box_val = [&](int n) -> float {
      if (!(y > 0 && n >= 4 * y && n < 4 * y + 4)) return 0.0f;
      const int j = n - 4 * y;
      const float dd = j == 0 ? d[0] : (j == 1 ? d[1] : (j == 2 ? d[2] : d[3]));
      return gbox * (dd < -1.0f ? -1.0f : (dd > 1.0f ? 1.0f : dd));
    };
    auto store = [&](float *gm, int q, const float *v) {
      float *o = gm + ((size_t)q * Mp + i) * 8;
      *reinterpret_cast<f32x4 *>(o) = f32x4{v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4 *>(o + 4) = f32x4{v[4], v[5], v[6], v[7]};
    };
    if (SPLIT) {
      for (int q = 0; q < (cb + 7) / 8; ++q) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = q * 8 + e < cb ? cls_val(q * 8 + e) : 0.0f;
        store(g, q, v);
      }
      for (int q = 0; q < (4 * C + 7) / 8; ++q) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = box_val(q * 8 + e);
        store(g_box, q, v);
      }
    } else {
      for (int q = 0; q < ((K + 4) * C + 7) / 8; ++q) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { const int n = q * 8 + e; v[e] = n < cb ? cls_val(n) : box_val(n - cb); }
        store(g, q, v);
      }
    }
  }
  s_cls[threadIdx.x] = acc_cls; s_box[threadIdx.x] = acc_box;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {  // a fixed tree: the same order in every run
    if ((int)threadIdx.x < w) { s_cls[threadIdx.x] += s_cls[threadIdx.x + w]; s_box[threadIdx.x] += s_box[threadIdx.x + w]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { loss[0] = s_cls[0] * invB; loss[1] = s_box[0] * gbox; }
}

int train_loss(const float *d_head, int B, int C, int K, int k, const float *d_rois, const float *d_gt, const int *d_labels, const LossCfg &cfg,
               float *d_g_c8, int Mp, float *d_loss, hipStream_t s) {
  MPN_CHECK_ARG(d_head && d_rois && d_gt && d_labels && d_g_c8 && d_loss && B > 0 && C > 1 && Mp >= B && K >= 1 && k >= 0 && k < K);
  const int ld = (K + 4) * C;
  hipLaunchKernelGGL(train_loss_kernel<false>, dim3(1), dim3(256), 0, s, d_head, ld, d_head + K * C, ld, B, C, K, k, d_rois, d_gt, d_labels, cfg, d_g_c8,
                     static_cast<float *>(nullptr), Mp, d_loss);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

int train_loss_split(const float *d_cls, const float *d_bbox, int B, int C, int K, int k, const float *d_rois, const float *d_gt, const int *d_labels,
                     const LossCfg &cfg, float *d_g_cls_c8, float *d_g_bbox_c8, int Mp, float *d_loss, hipStream_t s) {
  MPN_CHECK_ARG(d_cls && d_bbox && d_rois && d_gt && d_labels && d_g_cls_c8 && d_g_bbox_c8 && d_loss && B > 0 && C > 1 && Mp >= B && K >= 1 && k >= 0 && k < K);
  hipLaunchKernelGGL(train_loss_kernel<true>, dim3(1), dim3(256), 0, s, d_cls, K * C, d_bbox, 4 * C, B, C, K, k, d_rois, d_gt, d_labels, cfg, d_g_cls_c8,
                     d_g_bbox_c8, Mp, d_loss);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Weight gradient + SGD step on the packed weights
// ---------------------------------------------------------------------------------------------------------------------------------
struct SgdArgs {
  const float *g, *x;
  int g_Mp, x_Mp, B, N, K, inner, NP, nchunks;
  float *w, *v;
  float lr, mom, wd;
};

// Block = 4 waves side by side in n: 32 k-chunks (256 k) x 128 output rows n; a wave owns 32 chunks x 32 n.  A = x records (i = chunk),
// B = g[m][n] (j = n), contraction over the rows m in pairs (m0 + lane / 32).  For each of its 16 registers a lane then holds one whole
// record of dW — chunk ck0 + 8 (r / 4) + 4 (lane / 32) + r % 4, row n0 + lane % 32 — and streams w and v through it: per (r, half-wave) the
// wave reads and writes 1 KiB contiguous of each, the block 4 KiB (one packed chunk row is NP x 32 bytes).
__global__ __launch_bounds__(256, 2) void sgd_wgrad_kernel(SgdArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, half = lane >> 5;
  const int n = (blockIdx.x * 4 + wave) * 32 + l31;
  const int ck0 = blockIdx.y * 32, ck = ck0 + l31;
  const bool ck_ok = ck < a.nchunks, n_ok = n < a.N;
  f32x16 acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[e][r] = 0.0f;
  const float *xp = a.x + (size_t)(ck_ok ? ck : 0) * a.x_Mp * 8;
  const float *gp = a.g + (size_t)((n_ok ? n : 0) >> 3) * a.g_Mp * 8 + (n & 7);
  auto load = [&](int m0, f32x4 &lo, f32x4 &hi, float &b) {  // rows >= B contribute exact zeros on BOTH sides (stale rows may hold NaN)
    const int m = m0 + half;
    lo = f32x4{0.f, 0.f, 0.f, 0.f}; hi = lo; b = 0.0f;
    if (m < a.B) {
      if (ck_ok) { lo = *reinterpret_cast<const f32x4 *>(xp + (size_t)m * 8); hi = *reinterpret_cast<const f32x4 *>(xp + (size_t)m * 8 + 4); }
      if (n_ok) b = gp[(size_t)m * 8];
    }
  };
  f32x4 lo, hi; float b;
  load(0, lo, hi, b);
  for (int m0 = 0; m0 < a.B; m0 += 2) {
    f32x4 nlo, nhi; float nb;
    load(m0 + 2, nlo, nhi, nb);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(lo[e], b, acc[e], 0, 0, 0);
      acc[4 + e] = __builtin_amdgcn_mfma_f32_32x32x2f32(hi[e], b, acc[4 + e], 0, 0, 0);
    }
    lo = nlo; hi = nhi; b = nb;
  }
  if (!n_ok) return;  // pad rows of the packing stay +0.0
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int kc = ck0 + 8 * (r >> 2) + 4 * half + (r & 3);
    if (kc >= a.nchunks) continue;
    const size_t off = ((size_t)kc * a.NP + n) * 8;
    f32x4 w0 = *reinterpret_cast<const f32x4 *>(a.w + off), w1 = *reinterpret_cast<const f32x4 *>(a.w + off + 4);
    f32x4 v0 = *reinterpret_cast<const f32x4 *>(a.v + off), v1 = *reinterpret_cast<const f32x4 *>(a.v + off + 4);
    const long kbase = (long)(kc / a.inner) * 8 * a.inner + (kc % a.inner);  // k of float j: kbase + j * inner (pack_linear_weights)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (kbase + (long)e * a.inner < (long)a.K) {
        const float gr = acc[e][r] + a.wd * w0[e];
        v0[e] = a.mom * v0[e] + gr;
        w0[e] = w0[e] - a.lr * v0[e];
      }
      if (kbase + (long)(e + 4) * a.inner < (long)a.K) {
        const float gr = acc[4 + e][r] + a.wd * w1[e];
        v1[e] = a.mom * v1[e] + gr;
        w1[e] = w1[e] - a.lr * v1[e];
      }
    }
    *reinterpret_cast<f32x4 *>(a.w + off) = w0; *reinterpret_cast<f32x4 *>(a.w + off + 4) = w1;
    *reinterpret_cast<f32x4 *>(a.v + off) = v0; *reinterpret_cast<f32x4 *>(a.v + off + 4) = v1;
  }
}

int sgd_wgrad_c8(const float *d_g_c8, int g_Mp, const float *d_x_c8, int x_Mp, int B, int N, int K, int inner, float *d_wpk, float *d_vpk,
                 float lr, float momentum, float wd, hipStream_t s) {
  MPN_CHECK_ARG(d_g_c8 && d_x_c8 && d_wpk && d_vpk && B > 0 && N > 0 && K > 0 && inner > 0 && g_Mp >= B && x_Mp >= B);
  MPN_CHECK_ARG(inner == 1 || (K % (8 * inner)) == 0);
  SgdArgs a{};
  a.g = d_g_c8; a.x = d_x_c8; a.g_Mp = g_Mp; a.x_Mp = x_Mp; a.B = B; a.N = N; a.K = K; a.inner = inner;
  a.NP = lin_np(N); a.nchunks = round_up(K, 64) / 8;
  a.w = d_wpk; a.v = d_vpk; a.lr = lr; a.mom = momentum; a.wd = wd;
  hipLaunchKernelGGL(sgd_wgrad_kernel, dim3((unsigned)(a.NP / 128), (unsigned)cdiv(a.nchunks, 32)), dim3(256), 0, s, a);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// Block = one 8-column chunk of g: thread t sums column t % 8 over the rows m = t / 8 (mod 32), ascending, then a fixed LDS tree over the 32
// partial sums — a pairwise-style order (shorter error chains than one row-ascending sum), the same in every run.
__global__ __launch_bounds__(256) void sgd_bias_kernel(const float *__restrict__ g, int g_Mp, int B, int N, float *__restrict__ b, float *__restrict__ vb, float lr, float mom) {
  __shared__ float part[32][8];
  const int e = threadIdx.x & 7, slot = threadIdx.x >> 3, n = blockIdx.x * 8 + e;
  const float *gp = g + (size_t)blockIdx.x * g_Mp * 8 + e;
  float sum = 0.0f;
  for (int m = slot; m < B; m += 32) sum += gp[(size_t)m * 8];
  part[slot][e] = sum;
  __syncthreads();
  for (int w = 16; w > 0; w >>= 1) {
    if (slot < w) part[slot][e] += part[slot + w][e];
    __syncthreads();
  }
  if (slot != 0 || n >= N) return;
  const float v = mom * vb[n] + part[0][e];
  vb[n] = v;
  b[n] = b[n] - lr * v;
}

int sgd_bias_c8(const float *d_g_c8, int g_Mp, int B, int N, float *d_bpk, float *d_vb, float lr, float momentum, hipStream_t s) {
  MPN_CHECK_ARG(d_g_c8 && d_bpk && d_vb && B > 0 && N > 0 && g_Mp >= B);
  hipLaunchKernelGGL(sgd_bias_kernel, dim3((unsigned)cdiv(N, 8)), dim3(256), 0, s, d_g_c8, g_Mp, B, N, d_bpk, d_vb, lr, momentum);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The same two gradients over SEGMENTED rows: MultiPathNet's 1x1 mix layer, whose rows are (bin, roi) pairs
// ---------------------------------------------------------------------------------------------------------------------------------
struct SegWgradArgs {
  const float *g, *x;
  int Mp, B, N, NP, nchunks, rows_per_wave;
  size_t pitch;        // rows between two chunks of both operands: nseg * Mp
  float *part;
  size_t part_stride;  // floats between two segments' partial sums: nchunks * NP * 8
};

constexpr int kSegWgradLds = 2 * 128 * 64 * 4;  // two waves' accumulators

// sgd_wgrad_kernel's record mapping, one block per (32 k-chunks x 32 n tile, SEGMENT on grid.z).  The block's 4 waves cut the segment's B
// rows into four contiguous quarters (rows_per_wave, even): each accumulates its rows seg * Mp + m ascending in pairs from zero — rows
// >= B (stale, maybe NaN) contribute exact zeros on both sides — and the four sums are added pairwise through LDS, (q0 + q1) + (q2 + q3):
// chains of B / 8 MFMA steps instead of B / 2 (with one chain per bin the B = 128 gradient sat at 1.4 x the rms error of a blocked CPU
// sum, 2.3 x at its worst element).  The tile goes to the segment's slab of `part` in the packed layout; seg_wgrad_sgd_kernel adds the
// slabs.  A slab is written in full (all NP columns, all nchunks chunks), so the sum reads nothing stale.
__global__ __launch_bounds__(256, 2) void seg_wgrad_kernel(SegWgradArgs a) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, half = lane >> 5;
  const int n = blockIdx.x * 32 + l31;   // < NP: the grid covers NP exactly
  const int ck0 = blockIdx.y * 32, ck = ck0 + l31;
  const bool ck_ok = ck < a.nchunks, n_ok = n < a.N;
  const size_t row0 = (size_t)blockIdx.z * a.Mp;
  const int mb = wave * a.rows_per_wave, me = min(a.B, mb + a.rows_per_wave);
  f32x16 acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[e][r] = 0.0f;
  const float *xp = a.x + ((size_t)(ck_ok ? ck : 0) * a.pitch + row0) * 8;
  const float *gp = a.g + ((size_t)((n_ok ? n : 0) >> 3) * a.pitch + row0) * 8 + (n & 7);
  auto load = [&](int m0, f32x4 &lo, f32x4 &hi, float &b) {
    const int m = m0 + half;
    lo = f32x4{0.f, 0.f, 0.f, 0.f}; hi = lo; b = 0.0f;
    if (m < me) {
      if (ck_ok) { lo = *reinterpret_cast<const f32x4 *>(xp + (size_t)m * 8); hi = *reinterpret_cast<const f32x4 *>(xp + (size_t)m * 8 + 4); }
      if (n_ok) b = gp[(size_t)m * 8];
    }
  };
  f32x4 lo, hi; float b;
  load(mb, lo, hi, b);
  for (int m0 = mb; m0 < me; m0 += 2) {
    f32x4 nlo, nhi; float nb;
    load(m0 + 2, nlo, nhi, nb);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(lo[e], b, acc[e], 0, 0, 0);
      acc[4 + e] = __builtin_amdgcn_mfma_f32_32x32x2f32(hi[e], b, acc[4 + e], 0, 0, 0);
    }
    lo = nlo; hi = nhi; b = nb;
  }
  // (q0 + q1) and (q2 + q3): the odd waves hand their sums over, one 32 KiB slot each (lane-contiguous: no bank conflicts)
  auto put = [&](int slot) {
    float *o = lds + (size_t)slot * 128 * 64 + lane;
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[(e * 16 + r) * 64] = acc[e][r];
  };
  auto add = [&](int slot) {
    const float *o = lds + (size_t)slot * 128 * 64 + lane;
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[e][r] += o[(e * 16 + r) * 64];
  };
  if (wave & 1) put(wave >> 1);
  __syncthreads();
  if (!(wave & 1)) add(wave >> 1);
  __syncthreads();
  if (wave == 2) put(0);
  __syncthreads();
  if (wave != 0) return;
  add(0);
  float *out = a.part + (size_t)blockIdx.z * a.part_stride;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int kc = ck0 + 8 * (r >> 2) + 4 * half + (r & 3);
    if (kc >= a.nchunks) continue;
    const size_t off = ((size_t)kc * a.NP + n) * 8;
    *reinterpret_cast<f32x4 *>(out + off) = f32x4{acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
    *reinterpret_cast<f32x4 *>(out + off + 4) = f32x4{acc[4][r], acc[5][r], acc[6][r], acc[7][r]};
  }
}

// One thread per record (chunk kc, row n < N) of the packed weight: the segments' partial sums added in ascending order in groups of
// kWgradSegGroup, the group sums in ascending order (conv_wgrad_reduce_kernel's order), then optim.sgd on the record (inner = 1: float
// e is k = kc * 8 + e; lanes k >= K and rows n >= N keep the packing's +0.0).
__global__ __launch_bounds__(256) void seg_wgrad_sgd_kernel(const float *__restrict__ part, size_t stride, int nseg, int N, int NP, int K, int nchunks,
                                                            float *__restrict__ w, float *__restrict__ v, float lr, float mom, float wd) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)nchunks * NP) return;
  const int n = (int)(t % NP), kc = (int)(t / NP);
  if (n >= N || kc * 8 >= K) return;
  const size_t off = t * 8;
  f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = s0;
  for (int g0 = 0; g0 < nseg; g0 += kWgradSegGroup) {
    const int g1 = min(g0 + kWgradSegGroup, nseg);
    f32x4 q0 = f32x4{0.f, 0.f, 0.f, 0.f}, q1 = q0;
    for (int sg = g0; sg < g1; ++sg) {
      const float *pp = part + (size_t)sg * stride + off;
      q0 += *reinterpret_cast<const f32x4 *>(pp); q1 += *reinterpret_cast<const f32x4 *>(pp + 4);
    }
    if (g0 == 0) { s0 = q0; s1 = q1; } else { s0 += q0; s1 += q1; }
  }
  f32x4 w0 = *reinterpret_cast<const f32x4 *>(w + off), w1 = *reinterpret_cast<const f32x4 *>(w + off + 4);
  f32x4 v0 = *reinterpret_cast<const f32x4 *>(v + off), v1 = *reinterpret_cast<const f32x4 *>(v + off + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (kc * 8 + e < K) {
      const float gr = s0[e] + wd * w0[e];
      v0[e] = mom * v0[e] + gr;
      w0[e] = w0[e] - lr * v0[e];
    }
    if (kc * 8 + 4 + e < K) {
      const float gr = s1[e] + wd * w1[e];
      v1[e] = mom * v1[e] + gr;
      w1[e] = w1[e] - lr * v1[e];
    }
  }
  *reinterpret_cast<f32x4 *>(w + off) = w0; *reinterpret_cast<f32x4 *>(w + off + 4) = w1;
  *reinterpret_cast<f32x4 *>(v + off) = v0; *reinterpret_cast<f32x4 *>(v + off + 4) = v1;
}

size_t seg_wgrad_part_elems(int K, int N, int nseg) { return (size_t)nseg * (round_up(K, 64) / 8) * lin_np(N) * 8; }

int sgd_wgrad_seg_c8(const float *d_g_c8, const float *d_x_c8, int Mp, int nseg, int B, int N, int K, float *d_part, float *d_wpk, float *d_vpk,
                     float lr, float momentum, float wd, hipStream_t s) {
  MPN_CHECK_ARG(d_g_c8 && d_x_c8 && d_part && d_wpk && d_vpk && B > 0 && N > 0 && K > 0 && Mp >= B && nseg > 0 && nseg <= 65535);
  SegWgradArgs a{};
  a.g = d_g_c8; a.x = d_x_c8; a.Mp = Mp; a.B = B; a.N = N; a.NP = lin_np(N); a.nchunks = round_up(K, 64) / 8;
  a.rows_per_wave = round_up(cdiv(B, 4), 2);
  a.pitch = (size_t)nseg * Mp; a.part = d_part; a.part_stride = (size_t)a.nchunks * a.NP * 8;
  int rc = set_max_dyn_lds(reinterpret_cast<const void *>(seg_wgrad_kernel), kSegWgradLds);
  if (rc) return rc;
  hipLaunchKernelGGL(seg_wgrad_kernel, dim3((unsigned)(a.NP / 32), (unsigned)cdiv(a.nchunks, 32), (unsigned)nseg), dim3(256), kSegWgradLds, s, a);
  MPN_CHECK_LAUNCH();
  hipLaunchKernelGGL(seg_wgrad_sgd_kernel, dim3((unsigned)cdiv_sz((size_t)a.nchunks * a.NP, 256)), dim3(256), 0, s, d_part, a.part_stride, nseg, N, a.NP, K,
                     a.nchunks, d_wpk, d_vpk, lr, momentum, wd);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

constexpr int kSegBiasLds = 64 * 32 * 8 * 4;  // the slot sums of a block of 64 segments

// Block = one 8-column chunk of g.  Per segment sgd_bias_kernel's sum (thread t: column t % 8 over the rows seg * Mp + m, m = t / 8 mod 32,
// ascending, then the fixed LDS tree over the 32 partial sums); the segment sums then go through a second fixed tree (segments in
// blocks of 64 leaves, missing ones +0.0; the blocks' roots added in ascending order — one block for the 49 bins of a 7 x 7 pooling),
// and the one thread per column that holds the result takes the bias step.  The slot sums of a block of segments are all taken first
// and their trees run side by side: ten barriers per 64 segments.
__global__ __launch_bounds__(256) void seg_bias_sgd_kernel(const float *__restrict__ g, int Mp, int nseg, int B, int N, float *__restrict__ b,
                                                           float *__restrict__ vb, float lr, float mom) {
  extern __shared__ float sb[];  // [64 segments][32 slots][8]
  const int e = threadIdx.x & 7, slot = threadIdx.x >> 3, n = blockIdx.x * 8 + e;
  const float *gc = g + (size_t)blockIdx.x * nseg * Mp * 8 + e;
  float total = 0.0f;
  for (int s0 = 0; s0 < nseg; s0 += 64) {
    const int ns = min(64, nseg - s0);
    for (int sg = 0; sg < 64; ++sg) {
      float sum = 0.0f;
      if (sg < ns) {
        const float *gp = gc + (size_t)(s0 + sg) * Mp * 8;
        for (int m = slot; m < B; m += 32) sum += gp[(size_t)m * 8];
      }
      sb[(sg * 32 + slot) * 8 + e] = sum;
    }
    __syncthreads();
    for (int w = 16; w > 0; w >>= 1) {
      if (slot < w)
        for (int sg = 0; sg < ns; ++sg) sb[(sg * 32 + slot) * 8 + e] += sb[(sg * 32 + slot + w) * 8 + e];
      __syncthreads();
    }
    for (int w = 32; w > 0; w >>= 1) {  // the segment sums sb[sg][0]: leaves slot and slot + w
      if (slot < w) sb[slot * 32 * 8 + e] += sb[(slot + w) * 32 * 8 + e];
      __syncthreads();
    }
    if (slot == 0) total = s0 == 0 ? sb[e] : total + sb[e];
    __syncthreads();
  }
  if (slot != 0 || n >= N) return;
  const float v = mom * vb[n] + total;
  vb[n] = v;
  b[n] = b[n] - lr * v;
}

int sgd_bias_seg_c8(const float *d_g_c8, int Mp, int nseg, int B, int N, float *d_bpk, float *d_vb, float lr, float momentum, hipStream_t s) {
  MPN_CHECK_ARG(d_g_c8 && d_bpk && d_vb && B > 0 && N > 0 && Mp >= B && nseg > 0);
  int rc = set_max_dyn_lds(reinterpret_cast<const void *>(seg_bias_sgd_kernel), kSegBiasLds);
  if (rc) return rc;
  hipLaunchKernelGGL(seg_bias_sgd_kernel, dim3((unsigned)cdiv(N, 8)), dim3(256), kSegBiasLds, s, d_g_c8, Mp, nseg, B, N, d_bpk, d_vb, lr, momentum);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Input gradient: dx = scale * (g W) .* [act > 0]
// ---------------------------------------------------------------------------------------------------------------------------------
struct DgradArgs {
  const float *g, *w, *act;
  float *dx;
  int g_Mp, x_Mp, B, N, NP, nchunks, n_per_wave;
  float scale = 1.0f;  // of the masked value: 1 / (1 - rate) where a dropout sits behind the activation (x * 1.0f is x: the plain mask's bits)
};
constexpr int kDgradLds = 3 * 128 * 64 * 4;  // the partial sums of waves 1..3

// Block = 32 k-chunks (256 k) x 32 rows m; its 4 waves split the contraction over n into four contiguous ranges (n ascending in pairs
// inside a range) and wave 0 adds the four partial sums in wave order: ((s0 + s1) + s2) + s3, the same in every run.  A = packed-weight
// records (i = chunk; the record of (chunk, n) holds W[n][chunk * 8 .. + 8]), B = g[m][n] (j = m).  A lane of wave 0 ends with whole
// records of dx — chunk ck0 + 8 (r / 4) + 4 (lane / 32) + r % 4, row m0 + lane % 32 —, masks them with the forward activation, scales and stores.
__global__ __launch_bounds__(256) void linear_dgrad_kernel(DgradArgs a) {
  extern __shared__ float part[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, half = lane >> 5;
  const int ck0 = blockIdx.x * 32, ck = ck0 + l31;
  const int m = blockIdx.y * 32 + l31;
  const bool ck_ok = ck < a.nchunks, m_ok = m < a.B;
  f32x16 acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[e][r] = 0.0f;
  const int nb = wave * a.n_per_wave, ne = min(a.N, nb + a.n_per_wave);
  const float *wp = a.w + (size_t)(ck_ok ? ck : 0) * a.NP * 8;
  const float *gp = a.g + (size_t)(m_ok ? m : 0) * 8;
  auto load = [&](int n0, f32x4 &lo, f32x4 &hi, float &b) {
    const int n = n0 + half;
    lo = f32x4{0.f, 0.f, 0.f, 0.f}; hi = lo; b = 0.0f;
    if (n < ne) {
      if (ck_ok) { lo = *reinterpret_cast<const f32x4 *>(wp + (size_t)n * 8); hi = *reinterpret_cast<const f32x4 *>(wp + (size_t)n * 8 + 4); }
      if (m_ok) b = gp[(size_t)(n >> 3) * a.g_Mp * 8 + (n & 7)];
    }
  };
  f32x4 lo, hi; float b;
  load(nb, lo, hi, b);
  for (int n0 = nb; n0 < ne; n0 += 2) {
    f32x4 nlo, nhi; float nbv;
    load(n0 + 2, nlo, nhi, nbv);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(lo[e], b, acc[e], 0, 0, 0);
      acc[4 + e] = __builtin_amdgcn_mfma_f32_32x32x2f32(hi[e], b, acc[4 + e], 0, 0, 0);
    }
    lo = nlo; hi = nhi; b = nbv;
  }
  if (wave > 0) {
    float *o = part + (size_t)(wave - 1) * 128 * 64 + lane;
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[(e * 16 + r) * 64] = acc[e][r];
  }
  __syncthreads();
  if (wave > 0 || !m_ok) return;
#pragma unroll 1
  for (int w = 0; w < 3; ++w) {
    const float *o = part + (size_t)w * 128 * 64 + lane;
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[e][r] += o[(e * 16 + r) * 64];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int kc = ck0 + 8 * (r >> 2) + 4 * half + (r & 3);
    if (kc >= a.nchunks) continue;
    const size_t off = ((size_t)kc * a.x_Mp + m) * 8;
    f32x4 d0, d1;
    if (a.act) {
      const f32x4 a0 = *reinterpret_cast<const f32x4 *>(a.act + off), a1 = *reinterpret_cast<const f32x4 *>(a.act + off + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { d0[e] = a0[e] > 0.0f ? acc[e][r] * a.scale : 0.0f; d1[e] = a1[e] > 0.0f ? acc[4 + e][r] * a.scale : 0.0f; }
    } else {  // no activation behind the layer (MultiPathNet's 1x1 mix feeds fc6 directly): every element passes
#pragma unroll
      for (int e = 0; e < 4; ++e) { d0[e] = acc[e][r] * a.scale; d1[e] = acc[4 + e][r] * a.scale; }
    }
    *reinterpret_cast<f32x4 *>(a.dx + off) = d0; *reinterpret_cast<f32x4 *>(a.dx + off + 4) = d1;
  }
}

int linear_dgrad_c8(const float *d_g_c8, int g_Mp, int B, int N, const float *d_wpk, int K, const float *d_act_c8, float *d_dx_c8, int x_Mp,
                    hipStream_t s, float scale) {
  MPN_CHECK_ARG(d_g_c8 && d_wpk && d_dx_c8 && B > 0 && N > 0 && K > 0 && g_Mp >= B && x_Mp >= B);  // (d_act_c8 null: unmasked)
  DgradArgs a{};
  a.scale = scale;
  a.g = d_g_c8; a.w = d_wpk; a.act = d_act_c8; a.dx = d_dx_c8; a.g_Mp = g_Mp; a.x_Mp = x_Mp; a.B = B; a.N = N;
  a.NP = lin_np(N); a.nchunks = cdiv(K, 8);
  a.n_per_wave = round_up(cdiv(N, 4), 2);
  int rc = set_max_dyn_lds(reinterpret_cast<const void *>(linear_dgrad_kernel), kDgradLds);
  if (rc) return rc;
  hipLaunchKernelGGL(linear_dgrad_kernel, dim3((unsigned)cdiv(a.nchunks, 32), (unsigned)cdiv(B, 32)), dim3(256), kDgradLds, s, a);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Dropout behind fc6 / fc7 (the reference's default, train.lua:53 train_remove_dropouts = false)
// ---------------------------------------------------------------------------------------------------------------------------------
// (Philox4x32-10: philox.h, shared with the ROI sampler's draws)
// One thread = one record: row m < B of chunk q < ceil(N/8), i.e. columns 8q .. 8q + 7 = the Philox column groups 2q and 2q + 1.
// Threads run along m first: a wave reads and writes 2 KiB contiguous.
__global__ __launch_bounds__(256) void dropout_c8_kernel(float *__restrict__ y, int Mp, int B, int N, int nq, DropoutCfg c) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)nq * B) return;
  const int q = (int)(t / B), m = (int)(t % B);
  float *rec = y + ((size_t)q * Mp + m) * 8;
  uint32_t w[8];
  philox4x32_10((uint32_t)m, (uint32_t)(2 * q), c.layer, c.step, c.seed_lo, c.seed_hi, w);
  philox4x32_10((uint32_t)m, (uint32_t)(2 * q + 1), c.layer, c.step, c.seed_lo, c.seed_hi, w + 4);
  const f32x4 x0 = *reinterpret_cast<const f32x4 *>(rec), x1 = *reinterpret_cast<const f32x4 *>(rec + 4);
  f32x4 d0, d1;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    d0[e] = (w[e] >= c.threshold && q * 8 + e < N) ? x0[e] * c.scale : 0.0f;
    d1[e] = (w[4 + e] >= c.threshold && q * 8 + 4 + e < N) ? x1[e] * c.scale : 0.0f;
  }
  *reinterpret_cast<f32x4 *>(rec) = d0; *reinterpret_cast<f32x4 *>(rec + 4) = d1;
}

int dropout_c8(float *d_y_c8, int Mp, int B, int N, const DropoutCfg &cfg, hipStream_t s) {
  MPN_CHECK_ARG(d_y_c8 && B > 0 && N > 0 && Mp >= B);
  const int nq = cdiv(N, 8);
  hipLaunchKernelGGL(dropout_c8_kernel, dim3((unsigned)cdiv_sz((size_t)nq * B, 256)), dim3(256), 0, s, d_y_c8, Mp, B, N, nq, cfg);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The learning-rate drop's dfdx:mul(decay) (train.lua:321-335)
// ---------------------------------------------------------------------------------------------------------------------------------
// Grid-stride over the n4 = n / 4 float4 records, a wave reading and writing 1 KiB contiguous per trip; the n & 3 elements behind them
// go to the first threads of block 0 one by one.  No LDS, nothing but one multiply per element between the load and the store.
__global__ __launch_bounds__(256) void scale_momentum_kernel(float *__restrict__ v, size_t n4, int tail, float f) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  f32x4 *v4 = reinterpret_cast<f32x4 *>(v);
  for (size_t i = t0; i < n4; i += stride) {
    f32x4 x = v4[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = x[e] * f;
    v4[i] = x;
  }
  if (t0 < (size_t)tail) v[n4 * 4 + t0] = v[n4 * 4 + t0] * f;
}

constexpr unsigned kScaleMaxBlocks = 4096;  // 16 blocks of 256 threads per CU of an MI355X: the longest buffers take a few trips each

int scale_momentum(float *d_v, size_t n, float factor, hipStream_t s) {
  MPN_CHECK_ARG(d_v && n > 0 && ((uintptr_t)d_v & 15) == 0);
  const size_t n4 = n / 4;
  const unsigned blocks = (unsigned)std::min<size_t>(std::max<size_t>(cdiv_sz(n4, 256), 1), kScaleMaxBlocks);
  hipLaunchKernelGGL(scale_momentum_kernel, dim3(blocks), dim3(256), 0, s, d_v, n4, (int)(n & 3), factor);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

__global__ void c8_rows_to_rowmajor_kernel(const float *__restrict__ c8, int Mp, int M, int N, float *__restrict__ y) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)M * N) return;
  const int n = (int)(t % N), m = (int)(t / N);
  y[t] = c8[((size_t)(n >> 3) * Mp + m) * 8 + (n & 7)];
}

int c8_rows_to_rowmajor(const float *d_c8, int Mp, int M, int N, float *d_y, hipStream_t s) {
  MPN_CHECK_ARG(d_c8 && d_y && M > 0 && N > 0 && Mp >= M);
  hipLaunchKernelGGL(c8_rows_to_rowmajor_kernel, dim3((unsigned)cdiv_sz((size_t)M * N, 256)), dim3(256), 0, s, d_c8, Mp, M, N, d_y);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Packed weights back to Torch layout
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void unpack_lin_w_kernel(const float *__restrict__ wpk, const float *__restrict__ bpk, int K, int NP, int inner, int n0, int n1,
                                    float *__restrict__ w, float *__restrict__ b) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b && t < (size_t)(n1 - n0)) b[t] = bpk[n0 + t];
  if (!w || t >= (size_t)(n1 - n0) * K) return;
  const int n = n0 + (int)(t / K);
  const long k = (long)(t % K);
  const long u = k / inner, rem = k % inner;          // k = (q / inner * 8 + j) * inner + q % inner
  const long q = (u / 8) * inner + rem; const int j = (int)(u % 8);
  w[t] = wpk[((size_t)q * NP + n) * 8 + j];
}

int unpack_linear_weights(const float *d_wpk, const float *d_bpk, int K, int N, int inner, int n0, int n1, float *d_w, float *d_b, hipStream_t s) {
  MPN_CHECK_ARG(d_wpk && d_bpk && K > 0 && N > 0 && inner > 0 && n0 >= 0 && n1 > n0 && n1 <= N);
  MPN_CHECK_ARG(inner == 1 || (K % (8 * inner)) == 0);  // pack_linear_weights' rule: otherwise a k < K maps to a chunk past K64 / 8
  if (!d_w && !d_b) return MPN_OK;
  const size_t total = d_w ? (size_t)(n1 - n0) * K : (size_t)(n1 - n0);
  hipLaunchKernelGGL(unpack_lin_w_kernel, dim3((unsigned)cdiv_sz(total, 256)), dim3(256), 0, s, d_wpk, d_bpk, K, lin_np(N), inner, n0, n1, d_w, d_b);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// =================================================================================================================================
// The conv block above the last pooling layer (train.h)
// =================================================================================================================================
// One thread per (c, y, x) cell, x fastest: it walks the rows of its map and the bins in the contract's order and adds in that order.
__global__ __launch_bounds__(256) void roi_pool_backward_kernel(RoiBwd a) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)a.C * a.H * a.W) return;
  const int x = (int)(t % a.W), y = (int)((t / a.W) % a.H), c = (int)(t / ((size_t)a.W * a.H));
  const int b = blockIdx.y, cell = y * a.W + x, PP = a.PH * a.PW;
  const float *gc = a.g + (long)(c >> 3) * a.g_cb + (long)(c & 7) * a.g_c;
  float sum = 0.0f;
  for (int n = a.n0; n < a.n1; ++n) {
    const float *ro = a.rois + (size_t)n * 5;
    if (a.by_batch) {
      int rb = (int)ro[0] - 1;
      rb = rb < 0 ? 0 : (rb >= a.B ? a.B - 1 : rb);
      if (rb != b) continue;
    }
    unsigned phm = 0xffffffffu, pwm = 0xffffffffu;
    if (a.windows) {  // the bins whose window holds the cell: rows and columns of bins are independent in both bin rules
      phm = pwm = 0u;
      int hs, he, ws, we;
      for (int ph = 0; ph < a.PH; ++ph) {
        roi_bin_bounds(ro, a.scale, a.rr, a.H, a.W, a.PH, a.PW, ph, 0, hs, he, ws, we);
        if (y >= hs && y < he) phm |= 1u << ph;
      }
      if (!phm) continue;
      for (int pw = 0; pw < a.PW; ++pw) {
        roi_bin_bounds(ro, a.scale, a.rr, a.H, a.W, a.PH, a.PW, 0, pw, hs, he, ws, we);
        if (x >= ws && x < we) pwm |= 1u << pw;
      }
      if (!pwm) continue;
    }
    const int32_t *am = a.argmax + ((size_t)n * a.C + c) * PP;
    const float *gn = gc + (long)n * a.g_n;
    for (int ph = 0; ph < a.PH; ++ph) {
      if (!((phm >> (ph & 31)) & 1u)) continue;
      for (int pw = 0; pw < a.PW; ++pw) {
        if (!((pwm >> (pw & 31)) & 1u)) continue;
        const int bin = ph * a.PW + pw;
        if (am[bin] == cell) sum += gn[(long)bin * a.g_bin];
      }
    }
  }
  a.out[(long)b * a.o_b + (long)(c >> 3) * a.o_cb + (long)(c & 7) * a.o_c + (long)y * a.o_y + (long)x * a.o_x] = sum;
}

int roi_pool_backward(const RoiBwd &a, hipStream_t s) {
  MPN_CHECK_ARG(a.g && a.argmax && a.rois && a.out && a.B > 0 && a.C > 0 && a.H > 0 && a.W > 0 && a.PH > 0 && a.PW > 0 && a.n0 >= 0 && a.n1 >= a.n0);
  MPN_CHECK_ARG(a.by_batch || a.B == 1);
  MPN_CHECK_ARG(!a.windows || (a.PH <= 32 && a.PW <= 32));
  const size_t cells = (size_t)a.C * a.H * a.W;
  hipLaunchKernelGGL(roi_pool_backward_kernel, dim3((unsigned)cdiv_sz(cells, 256), (unsigned)a.B), dim3(256), 0, s, a);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 3x3 convolution weight gradient
// ---------------------------------------------------------------------------------------------------------------------------------
struct ConvWgradArgs {
  const float *x, *g;
  size_t plane, part_stride;
  int Wp, H, W, Cout, CoutP, nq;
  float *part;
};

// sgd_wgrad_kernel's record mapping on a convolution.  The `wpk` layout [chunk][tap][CoutP][8] is a packed linear weight whose K chunks are
// the pairs q = chunk * 9 + tap: A = the 32-byte record of X's channel chunk at the pixel shifted by the tap (i = q, 32 of them per
// block), B = G[co][pixel] (j = co, 4 waves x 32), contraction over the pixels of the block's segment, row-major, in pairs (pixel
// p0 + 2 s + lane / 32).  A lane ends with whole `wpk` records of the segment's partial dW: q0 + 8 (r / 4) + 4 (lane / 32) + r % 4, cout co.
// Grid: (CoutP / 128, ceil(nq / 32), segments).  Nothing outside the H x W interior of G is read; X is read one cell into its halo.
__global__ __launch_bounds__(256, 2) void conv3x3_wgrad_kernel(ConvWgradArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, half = lane >> 5;
  const int co0 = (blockIdx.x * 4 + wave) * 32, co = co0 + l31;
  if (co0 >= a.Cout) return;  // (wave-uniform) a wave of pad couts only
  const int q0 = blockIdx.y * 32, q = q0 + l31;
  const bool q_ok = q < a.nq, co_ok = co < a.Cout;
  const int HW = a.H * a.W, p0 = blockIdx.z * kWgradSegPx, p1 = min(p0 + kWgradSegPx, HW);
  f32x16 acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[e][r] = 0.0f;
  const int qq = q_ok ? q : 0, chunk = qq / 9, tap = qq - chunk * 9, ky = tap / 3, kx = tap - ky * 3;
  const float *xp = a.x + (size_t)chunk * a.plane + ((size_t)ky * a.Wp + kx) * 8;           // cell (y + ky - 1, x + kx - 1) of pixel (y, x)
  const float *gp = a.g + (size_t)((co_ok ? co : 0) >> 3) * a.plane + ((size_t)a.Wp + 1) * 8 + (co & 7);
  auto load = [&](int m0, f32x4 &lo, f32x4 &hi, float &b) {  // pixels >= p1 contribute exact zeros on both sides
    const int pi = m0 + half;
    lo = f32x4{0.f, 0.f, 0.f, 0.f}; hi = lo; b = 0.0f;
    if (pi < p1) {
      const int y = pi / a.W, x = pi - y * a.W;
      const size_t off = ((size_t)y * a.Wp + x) * 8;
      if (q_ok) { lo = *reinterpret_cast<const f32x4 *>(xp + off); hi = *reinterpret_cast<const f32x4 *>(xp + off + 4); }
      if (co_ok) b = gp[off];
    }
  };
  f32x4 lo, hi; float b;
  load(p0, lo, hi, b);
  for (int m0 = p0; m0 < p1; m0 += 2) {
    f32x4 nlo, nhi; float nb;
    load(m0 + 2, nlo, nhi, nb);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(lo[e], b, acc[e], 0, 0, 0);
      acc[4 + e] = __builtin_amdgcn_mfma_f32_32x32x2f32(hi[e], b, acc[4 + e], 0, 0, 0);
    }
    lo = nlo; hi = nhi; b = nb;
  }
  if (!co_ok) return;
  float *part = a.part + (size_t)blockIdx.z * a.part_stride;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qr = q0 + 8 * (r >> 2) + 4 * half + (r & 3);
    if (qr >= a.nq) continue;
    float *o = part + ((size_t)qr * a.CoutP + co) * 8;
    *reinterpret_cast<f32x4 *>(o) = f32x4{acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
    *reinterpret_cast<f32x4 *>(o + 4) = f32x4{acc[4][r], acc[5][r], acc[6][r], acc[7][r]};
  }
}

// dW (+)= (g[0] + g[1]) + ... with g[i] = ((part[8 i] + part[8 i + 1]) + ...) + part[8 i + 7] (train.h kWgradSegGroup); lanes outside the layer get
// +0.0 without a read of `part`: the records of pad couts are never written by the kernel above (stale), the pad-cin lanes of a real
// cout's record hold its sums over X's pad channels
__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(const float *__restrict__ part, size_t stride, int nseg, int Cin, int Cout, int CoutP,
                                                                size_t total, float *__restrict__ dw, int accumulate) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int e = (int)(t & 7);
  const size_t r = t >> 3;
  const int co = (int)(r % CoutP), q = (int)(r / CoutP), ci = (q / 9) * 8 + e;
  float v = 0.0f;
  if (co < Cout && ci < Cin) {
    for (int g0 = 0; g0 < nseg; g0 += kWgradSegGroup) {  // groups of segments, each summed from zero in ascending order
      const int g1 = min(g0 + kWgradSegGroup, nseg);
      float gs = 0.0f;
      for (int sg = g0; sg < g1; ++sg) gs += part[(size_t)sg * stride + t];
      v = g0 == 0 ? gs : v + gs;
    }
    if (accumulate) v = dw[t] + v;
  }
  dw[t] = v;
}

size_t conv_wgrad_part_elems(int Cin, int Cout, int H, int W) { return (size_t)cdiv(H * W, kWgradSegPx) * conv_wpk_elems(Cin, Cout); }

int conv3x3_wgrad(const Act &x, const Act &g, float *d_part, float *d_dw, int accumulate, hipStream_t s) {
  MPN_CHECK_ARG(x.p && g.p && d_part && d_dw && x.H == g.H && x.W == g.W && x.Hp == g.Hp && x.Wp == g.Wp && x.H > 0 && x.W > 0);
  ConvWgradArgs a{};
  a.x = x.p; a.g = g.p; a.plane = x.plane(); a.Wp = x.Wp; a.H = x.H; a.W = x.W;
  a.Cout = g.C; a.CoutP = conv_coutp(g.C); a.nq = x.Cb() * 9;
  a.part = d_part; a.part_stride = conv_wpk_elems(x.C, g.C);
  const int nseg = cdiv(x.H * x.W, kWgradSegPx);
  hipLaunchKernelGGL(conv3x3_wgrad_kernel, dim3((unsigned)(a.CoutP / 128), (unsigned)cdiv(a.nq, 32), (unsigned)nseg), dim3(256), 0, s, a);
  MPN_CHECK_LAUNCH();
  const size_t total = a.part_stride;
  hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3((unsigned)cdiv_sz(total, 256)), dim3(256), 0, s, d_part, a.part_stride, nseg, x.C, g.C, a.CoutP,
                     total, d_dw, accumulate);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// Block = one 8-channel block of G: thread t sums channel t % 8 over the pixels t / 8 (mod 32) of the row-major interior, ascending, then
// a fixed LDS tree over the 32 partial sums (sgd_bias_kernel's order, over pixels)
__global__ __launch_bounds__(256) void conv_bias_grad_kernel(const float *__restrict__ g, size_t plane, int Wp, int H, int W, int Cout,
                                                             float *__restrict__ db, int accumulate) {
  __shared__ float part[32][8];
  const int e = threadIdx.x & 7, slot = threadIdx.x >> 3, co = blockIdx.x * 8 + e;
  const float *gp = g + (size_t)blockIdx.x * plane + ((size_t)Wp + 1) * 8 + e;
  float sum = 0.0f;
  for (int pi = slot; pi < H * W; pi += 32) {
    const int y = pi / W, x = pi - y * W;
    sum += gp[((size_t)y * Wp + x) * 8];
  }
  part[slot][e] = sum;
  __syncthreads();
  for (int w = 16; w > 0; w >>= 1) {
    if (slot < w) part[slot][e] += part[slot + w][e];
    __syncthreads();
  }
  if (slot != 0 || co >= Cout) return;
  db[co] = accumulate ? db[co] + part[0][e] : part[0][e];
}

int conv_bias_grad(const Act &g, float *d_db, int accumulate, hipStream_t s) {
  MPN_CHECK_ARG(g.p && d_db && g.H > 0 && g.W > 0);
  hipLaunchKernelGGL(conv_bias_grad_kernel, dim3((unsigned)g.Cb()), dim3(256), 0, s, g.p, g.plane(), g.Wp, g.H, g.W, g.C, d_db, accumulate);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

__global__ __launch_bounds__(256) void relu_mask_c8p_kernel(float *__restrict__ g, const float *__restrict__ x, int Cb, size_t plane, int Wp, int H, int W) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // one half-record per thread
  if (t >= (size_t)Cb * H * W * 2) return;
  const int h = (int)(t & 1);
  const size_t r = t >> 1;
  const int px = (int)(r % W), py = (int)((r / W) % H), cb = (int)(r / ((size_t)W * H));
  const size_t off = (size_t)cb * plane + ((size_t)(py + 1) * Wp + px + 1) * 8 + h * 4;
  const f32x4 xv = *reinterpret_cast<const f32x4 *>(x + off);
  f32x4 gv = *reinterpret_cast<const f32x4 *>(g + off);
#pragma unroll
  for (int e = 0; e < 4; ++e) gv[e] = xv[e] > 0.0f ? gv[e] : 0.0f;
  *reinterpret_cast<f32x4 *>(g + off) = gv;
}

int relu_mask_c8p(const Act &g, const Act &x, hipStream_t s) {
  MPN_CHECK_ARG(g.p && x.p && g.C == x.C && g.H == x.H && g.W == x.W && g.Hp == x.Hp && g.Wp == x.Wp);
  const size_t total = (size_t)g.Cb() * g.H * g.W * 2;
  hipLaunchKernelGGL(relu_mask_c8p_kernel, dim3((unsigned)cdiv_sz(total, 256)), dim3(256), 0, s, g.p, x.p, g.Cb(), g.plane(), g.Wp, g.H, g.W);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 2x2 ceil-mode max-pool backward (+ the ReLU mask of the pre-pool map)
// ---------------------------------------------------------------------------------------------------------------------------------
template <int V>
__device__ __forceinline__ void pool_load(const float *p, float (&v)[V]) {
  if constexpr (V == 8) {
    const f32x4 lo = *reinterpret_cast<const f32x4 *>(p), hi = *reinterpret_cast<const f32x4 *>(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = lo[e]; v[4 + e] = hi[e]; }
  } else {
    v[0] = p[0];
  }
}
template <int V>
__device__ __forceinline__ void pool_store(float *p, const float (&v)[V]) {
  if constexpr (V == 8) {
    *reinterpret_cast<f32x4 *>(p) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4 *>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
  } else {
    p[0] = v[0];
  }
}

// One thread per (channel block, window), windows along x fastest: with C8P operands a wave reads 64 windows = 128 consecutive records
// (4 KiB) of each of the two rows of X, 2 KiB of dY, and writes the same 2 x 4 KiB of dX.  Cells outside the map (ceil mode: the last
// row / column of windows of an odd size) are neither read nor written.
template <int V>
__global__ __launch_bounds__(256) void maxpool2x2_backward_kernel(PoolBwd a) {
  const int Ho = (a.H + 1) / 2, Wo = (a.W + 1) / 2;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)a.CB * Ho * Wo) return;
  const int X = (int)(t % Wo), Y = (int)((t / Wo) % Ho), cb = (int)(t / ((size_t)Wo * Ho));
  const int y0 = 2 * Y, x0 = 2 * X;
  const bool in[4] = {true, x0 + 1 < a.W, y0 + 1 < a.H, x0 + 1 < a.W && y0 + 1 < a.H};   // the forward's scan order
  const float *xp = a.x + (long)cb * a.x_cb + (long)y0 * a.x_y + (long)x0 * a.x_x;
  float v[4][V], g[V], o[4][V];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (in[q]) pool_load<V>(xp + (long)(q >> 1) * a.x_y + (long)(q & 1) * a.x_x, v[q]);
    else {
#pragma unroll
      for (int e = 0; e < V; ++e) v[q][e] = 0.0f;
    }
  }
  pool_load<V>(a.dy + (long)cb * a.g_cb + (long)Y * a.g_y + (long)X * a.g_x, g);
#pragma unroll
  for (int e = 0; e < V; ++e) {
    float m = -INFINITY;
    int win = -1;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (in[q] && v[q][e] > m) { m = v[q][e]; win = q; }
    if (a.relu_mask && !(m > 0.0f)) win = -1;
    if (cb * V + e >= a.C) win = -1;   // pad lanes of the last channel block
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q][e] = win == q ? g[e] : 0.0f;
  }
  float *dp = a.dx + (long)cb * a.d_cb + (long)y0 * a.d_y + (long)x0 * a.d_x;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (in[q]) pool_store<V>(dp + (long)(q >> 1) * a.d_y + (long)(q & 1) * a.d_x, o[q]);
}

int maxpool2x2_backward(const PoolBwd &a, hipStream_t s) {
  MPN_CHECK_ARG(a.x && a.dy && a.dx && a.CB > 0 && a.C > 0 && a.H > 0 && a.W > 0 && (a.vec == 1 || a.vec == 8));
  MPN_CHECK_ARG(a.C <= a.CB * a.vec && a.C > (a.CB - 1) * a.vec);
  const size_t total = (size_t)a.CB * ((a.H + 1) / 2) * ((a.W + 1) / 2);
  const dim3 grid((unsigned)cdiv_sz(total, 256));
  if (a.vec == 8) hipLaunchKernelGGL(maxpool2x2_backward_kernel<8>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(maxpool2x2_backward_kernel<1>, grid, dim3(256), 0, s, a);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

int maxpool2x2_backward_c8p(const Act &x, const Act &dy, const Act &dx, int relu_mask, hipStream_t s) {
  MPN_CHECK_ARG(x.p && dy.p && dx.p && x.C == dy.C && x.C == dx.C && dx.H == x.H && dx.W == x.W && dx.Hp == x.Hp && dx.Wp == x.Wp);
  MPN_CHECK_ARG(dy.H == (x.H + 1) / 2 && dy.W == (x.W + 1) / 2);
  PoolBwd a{};
  a.x = x.p + ((size_t)x.Wp + 1) * 8; a.dy = dy.p + ((size_t)dy.Wp + 1) * 8; a.dx = dx.p + ((size_t)dx.Wp + 1) * 8;
  a.vec = 8; a.CB = x.Cb(); a.C = x.C; a.H = x.H; a.W = x.W; a.relu_mask = relu_mask;
  a.x_cb = (long)x.plane(); a.x_y = (long)x.Wp * 8; a.x_x = 8;
  a.g_cb = (long)dy.plane(); a.g_y = (long)dy.Wp * 8; a.g_x = 8;
  a.d_cb = (long)dx.plane(); a.d_y = (long)dx.Wp * 8; a.d_x = 8;
  return maxpool2x2_backward(a, s);
}

__global__ __launch_bounds__(256) void conv_sgd_kernel(float *__restrict__ w, float *__restrict__ v, const float *__restrict__ dw, int Cin, int Cout,
                                                       int CoutP, size_t total, float lr, float mom, float wd) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const size_t r = t >> 3;
  const int co = (int)(r % CoutP), q = (int)(r / CoutP), ci = (q / 9) * 8 + (int)(t & 7);
  if (co >= Cout || ci >= Cin) return;  // pad lanes of the packing stay +0.0
  const float wv = w[t];
  const float gr = dw[t] + wd * wv;
  const float vv = mom * v[t] + gr;
  v[t] = vv;
  w[t] = wv - lr * vv;
}

int conv_sgd(float *d_wpk, float *d_vpk, const float *d_dw, int Cin, int Cout, float lr, float momentum, float wd, hipStream_t s) {
  MPN_CHECK_ARG(d_wpk && d_vpk && d_dw && Cin > 0 && Cout > 0);
  const size_t total = conv_wpk_elems(Cin, Cout);
  hipLaunchKernelGGL(conv_sgd_kernel, dim3((unsigned)cdiv_sz(total, 256)), dim3(256), 0, s, d_wpk, d_vpk, d_dw, Cin, Cout, conv_coutp(Cout), total, lr,
                     momentum, wd);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

__global__ void vec_sgd_kernel(float *__restrict__ b, float *__restrict__ vb, const float *__restrict__ db, int n, float lr, float mom) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const float v = mom * vb[t] + db[t];
  vb[t] = v;
  b[t] = b[t] - lr * v;
}

int vec_sgd(float *d_b, float *d_vb, const float *d_db, int n, float lr, float momentum, hipStream_t s) {
  MPN_CHECK_ARG(d_b && d_vb && d_db && n > 0);
  hipLaunchKernelGGL(vec_sgd_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, d_b, d_vb, d_db, n, lr, momentum);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

__global__ void unpack_conv_w_kernel(const float *__restrict__ wpk, const float *__restrict__ bpk, int Cin, int Cout, int CoutP,
                                     float *__restrict__ w, float *__restrict__ b) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b && t < (size_t)Cout) b[t] = bpk[t];
  if (!w || t >= (size_t)Cout * Cin * 9) return;
  const int tap = (int)(t % 9), ci = (int)((t / 9) % Cin), co = (int)(t / ((size_t)9 * Cin));
  w[t] = wpk[(((size_t)(ci >> 3) * 9 + tap) * CoutP + co) * 8 + (ci & 7)];
}

int unpack_conv_weights(const float *d_wpk, const float *d_bpk, int Cin, int Cout, float *d_w, float *d_b, hipStream_t s) {
  MPN_CHECK_ARG(d_wpk && (d_bpk || !d_b) && Cin > 0 && Cout > 0);
  if (!d_w && !d_b) return MPN_OK;
  const size_t total = d_w ? (size_t)Cout * Cin * 9 : (size_t)Cout;
  hipLaunchKernelGGL(unpack_conv_w_kernel, dim3((unsigned)cdiv_sz(total, 256)), dim3(256), 0, s, d_wpk, d_bpk, Cin, Cout, conv_coutp(Cout), d_w, d_b);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// W'[ci][co][2 - ky][2 - kx] = W[co][ci][ky][kx]: the `wpk` pack of the Cout -> Cin convolution that computes the input gradient, its
// zero bias, and (wt non-null) W' in Torch layout for the Winograd packer
__global__ void pack_conv_w_dgrad_kernel(const float *__restrict__ w, int Cin, int Cout, int CinP, int nchunks, float *__restrict__ wpk_t,
                                         float *__restrict__ zero_b, float *__restrict__ wt) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < (size_t)CinP) zero_b[t] = 0.0f;
  if (wt && t < (size_t)Cout * Cin * 9) {
    const int tap = (int)(t % 9), co = (int)((t / 9) % Cout), ci = (int)(t / ((size_t)9 * Cout));
    wt[t] = w[((size_t)co * Cin + ci) * 9 + (8 - tap)];
  }
  if (t >= (size_t)nchunks * 9 * CinP * 8) return;
  const int j = (int)(t & 7);
  size_t r = t >> 3;
  const int ci = (int)(r % CinP); r /= CinP;
  const int tap = (int)(r % 9), co = (int)(r / 9) * 8 + j;
  wpk_t[t] = (ci < Cin && co < Cout) ? w[((size_t)co * Cin + ci) * 9 + (8 - tap)] : 0.0f;
}

int pack_conv_weights_dgrad(const float *d_w, int Cin, int Cout, float *d_tmp, float *d_wpk_t, float *d_zero_b, float *d_wino_t, hipStream_t s) {
  MPN_CHECK_ARG(d_w && d_wpk_t && d_zero_b && Cin > 0 && Cout > 0 && (d_tmp || !d_wino_t));
  const int nchunks = (Cout + 7) / 8, CinP = conv_coutp(Cin);
  size_t total = (size_t)nchunks * 9 * CinP * 8;
  if (d_wino_t && (size_t)Cout * Cin * 9 > total) total = (size_t)Cout * Cin * 9;
  hipLaunchKernelGGL(pack_conv_w_dgrad_kernel, dim3((unsigned)cdiv_sz(total, 256)), dim3(256), 0, s, d_w, Cin, Cout, CinP, nchunks, d_wpk_t, d_zero_b,
                     d_wino_t ? d_tmp : nullptr);
  MPN_CHECK_LAUNCH();
  return d_wino_t ? pack_conv_weights_wino(d_tmp, Cout, Cin, d_wino_t, s) : MPN_OK;
}

// =================================================================================================================================
// MultiPathNet's conv5 block through the skip pooling (train.h)
// =================================================================================================================================
// One block per row.  Pass 1: thread t walks its entries ascending (stride 256 floats = 32 records: a wave reads 8 records of 32 bytes,
// Mp * 32 bytes apart — the layout's row pitch, not the kernel's choice) into two partial sums, the LDS tree adds them.  Pass 2: the
// same walk, elementwise.  y and g are read twice (the second time from L2), x once, dx is written once.
__global__ __launch_bounds__(kNormBwdThreads) void normalize_backward_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ g, float *__restrict__ dx,
                                                                             int Mp, int C, int PP, int E, float mul) {
  __shared__ float pss[kNormBwdThreads], pd[kNormBwdThreads];
  const int t = threadIdx.x;
  const size_t n8 = (size_t)blockIdx.x * 8;
  float ss = 0.0f, d = 0.0f;
  for (int e = t; e < E; e += kNormBwdThreads) {
    const int r = e >> 3, lane = e & 7;
    if ((r / PP) * 8 + lane >= C) continue;  // a pad lane of the last channel block
    const size_t off = (size_t)r * Mp * 8 + n8 + lane;
    const float xv = x[off];
    ss = fmaf(xv, xv, ss);
    d = fmaf(y[off], g[off], d);
  }
  pss[t] = ss; pd[t] = d;
  __syncthreads();
  for (int h = kNormBwdThreads / 2; h >= 1; h >>= 1) {
    if (t < h) { pss[t] += pss[t + h]; pd[t] += pd[t + h]; }
    __syncthreads();
  }
  const float sc = mul / sqrtf(pss[0] + 1e-10f), coef = pd[0] / (mul * mul);
  for (int e = t; e < E; e += kNormBwdThreads) {
    const int r = e >> 3, lane = e & 7;
    if ((r / PP) * 8 + lane >= C) continue;
    const size_t off = (size_t)r * Mp * 8 + n8 + lane;
    dx[off] = sc * (g[off] - y[off] * coef);
  }
}

int normalize_backward_c8(const float *d_x_c8, const float *d_y_c8, const float *d_g_c8, float *d_dx_c8, int Mp, int B, int C, int PP, float mul, hipStream_t s) {
  MPN_CHECK_ARG(d_x_c8 && d_y_c8 && d_g_c8 && d_dx_c8 && B > 0 && Mp >= B && C > 0 && PP > 0 && mul > 0.0f);
  hipLaunchKernelGGL(normalize_backward_kernel, dim3((unsigned)B), dim3(kNormBwdThreads), 0, s, d_x_c8, d_y_c8, d_g_c8, d_dx_c8, Mp, C, PP, cdiv(C, 8) * PP * 8, mul);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// roi_pool_backward_kernel's walk for one map and one tower's region, the chain continued from the cell's value (train.h).  One thread
// per (c, y, x) cell, x fastest; the cell's own record lane is read and written by this thread alone.
__global__ __launch_bounds__(256) void roi_pool_backward_add_kernel(RoiBwd a, int roi_stride) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)a.C * a.H * a.W) return;
  const int x = (int)(t % a.W), y = (int)((t / a.W) % a.H), c = (int)(t / ((size_t)a.W * a.H));
  const int cell = y * a.W + x, PP = a.PH * a.PW;
  const float *gc = a.g + (long)(c >> 3) * a.g_cb + (long)(c & 7) * a.g_c;
  float *o = a.out + (long)(c >> 3) * a.o_cb + (long)(c & 7) * a.o_c + (long)y * a.o_y + (long)x * a.o_x;
  float sum = *o;
  for (int n = a.n0; n < a.n1; ++n) {
    const float *ro = a.rois + (size_t)n * roi_stride;
    unsigned phm = 0xffffffffu, pwm = 0xffffffffu;
    if (a.windows) {
      phm = pwm = 0u;
      int hs, he, ws, we;
      for (int ph = 0; ph < a.PH; ++ph) {
        roi_bin_bounds(ro, a.scale, a.rr, a.H, a.W, a.PH, a.PW, ph, 0, hs, he, ws, we);
        if (y >= hs && y < he) phm |= 1u << ph;
      }
      if (!phm) continue;
      for (int pw = 0; pw < a.PW; ++pw) {
        roi_bin_bounds(ro, a.scale, a.rr, a.H, a.W, a.PH, a.PW, 0, pw, hs, he, ws, we);
        if (x >= ws && x < we) pwm |= 1u << pw;
      }
      if (!pwm) continue;
    }
    const int32_t *am = a.argmax + ((size_t)n * a.C + c) * PP;
    const float *gn = gc + (long)n * a.g_n;
    for (int ph = 0; ph < a.PH; ++ph) {
      if (!((phm >> (ph & 31)) & 1u)) continue;
      for (int pw = 0; pw < a.PW; ++pw) {
        if (!((pwm >> (pw & 31)) & 1u)) continue;
        const int bin = ph * a.PW + pw;
        if (am[bin] == cell) sum += gn[(long)bin * a.g_bin];
      }
    }
  }
  *o = sum;
}

int roi_pool_backward_add(const RoiBwd &a, int roi_stride, hipStream_t s) {
  MPN_CHECK_ARG(a.g && a.argmax && a.rois && a.out && a.B == 1 && !a.by_batch && a.C > 0 && a.H > 0 && a.W > 0 && a.PH > 0 && a.PW > 0 && a.n0 >= 0 && a.n1 >= a.n0);
  MPN_CHECK_ARG(roi_stride >= 5 && (!a.windows || (a.PH <= 32 && a.PW <= 32)));
  const size_t cells = (size_t)a.C * a.H * a.W;
  hipLaunchKernelGGL(roi_pool_backward_add_kernel, dim3((unsigned)cdiv_sz(cells, 256)), dim3(256), 0, s, a, roi_stride);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

__global__ void int_to_float_kernel(const int32_t *__restrict__ in, size_t n, float *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (float)in[i];
}

int int_to_float(const int32_t *d_in, size_t n, float *d_out, hipStream_t s) {
  MPN_CHECK_ARG(d_in && d_out && n > 0);
  hipLaunchKernelGGL(int_to_float_kernel, dim3((unsigned)cdiv_sz(n, 256)), dim3(256), 0, s, d_in, n, d_out);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

}  // namespace mpn

// ---- module-level C entry points (NCHW Torch layouts) -----------------------------------------------------------------------------
using namespace mpn;

extern "C" int mpn_roi_pool_backward(const float *d_grad_out, const int32_t *d_argmax, const float *d_rois, int B, int C, int H, int W, int N,
                                     int PH, int PW, float *d_grad_in, void *stream) {
  MPN_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && PH > 0 && PW > 0 && N >= 0 && d_grad_in);
  MPN_CHECK_ARG(N == 0 || (d_grad_out && d_argmax && d_rois));
  if (N == 0) { MPN_CHECK_HIP(hipMemsetAsync(d_grad_in, 0, (size_t)B * C * H * W * sizeof(float), as_stream(stream))); return MPN_OK; }
  RoiBwd a{};
  const long PP = (long)PH * PW;
  a.g = d_grad_out; a.argmax = d_argmax; a.rois = d_rois; a.by_batch = 1; a.n0 = 0; a.n1 = N; a.B = B; a.C = C; a.H = H; a.W = W; a.PH = PH; a.PW = PW;
  a.g_n = (long)C * PP; a.g_cb = 8 * PP; a.g_c = PP; a.g_bin = 1;
  a.o_b = (long)C * H * W; a.o_cb = 8L * H * W; a.o_c = (long)H * W; a.o_y = W; a.o_x = 1;
  a.out = d_grad_in;
  return roi_pool_backward(a, as_stream(stream));
}

extern "C" int mpn_maxpool2x2_ceil_backward(const float *d_in, const float *d_grad_out, int BC, int H, int W, int relu_mask, float *d_grad_in,
                                            void *stream) {
  MPN_CHECK_ARG(d_in && d_grad_out && d_grad_in && BC > 0 && H > 0 && W > 0);
  const long Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  PoolBwd a{};
  a.x = d_in; a.dy = d_grad_out; a.dx = d_grad_in;
  a.vec = 1; a.CB = BC; a.C = BC; a.H = H; a.W = W; a.relu_mask = relu_mask != 0;
  a.x_cb = (long)H * W; a.x_y = W; a.x_x = 1;
  a.g_cb = Ho * Wo; a.g_y = Wo; a.g_x = 1;
  a.d_cb = (long)H * W; a.d_y = W; a.d_x = 1;
  return maxpool2x2_backward(a, as_stream(stream));
}

static bool dgrad_has_wino(int Cout) { return Cout >= 16; }  // build_vgg_trunk's rule on the transposed layer (its input channels = Cout)

extern "C" size_t mpn_conv3x3_backward_workspace_bytes(int B, int Cin, int H, int W, int Cout) {
  (void)B;
  const size_t acts = 2 * act_bytes(Cin, H, W) + act_bytes(Cout, H, W);
  const size_t w = ((size_t)Cout * Cin * 9 + conv_wpk_elems(Cout, Cin) + conv_wino_elems(Cout, Cin) + (size_t)conv_coutp(Cin) +
                    conv_wpk_elems(Cin, Cout) + (size_t)conv_coutp(Cout) + conv_wgrad_part_elems(Cin, Cout, H, W)) * sizeof(float);
  return acts + w + 1024;
}

extern "C" int mpn_conv3x3_backward(const float *d_in, int B, int Cin, int H, int W, const float *d_w, const float *d_grad_out, int Cout,
                                    float *d_grad_in, float *d_grad_w, float *d_grad_b, void *d_ws, size_t ws_bytes, void *stream) {
  MPN_CHECK_ARG(d_grad_out && d_ws && B > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0);
  MPN_CHECK_ARG((d_in || !d_grad_w) && (d_w || !d_grad_in));
  const size_t need = mpn_conv3x3_backward_workspace_bytes(B, Cin, H, W, Cout);
  if (ws_bytes < need) { set_error("mpn_conv3x3_backward: workspace too small (%zu < %zu)", ws_bytes, need); return MPN_ENOMEM; }
  hipStream_t s = as_stream(stream);
  char *ws = static_cast<char *>(d_ws);
  const size_t ab = act_bytes(Cin, H, W), gb = act_bytes(Cout, H, W);
  Act ax = make_act(reinterpret_cast<float *>(ws), Cin, H, W);
  Act adx = make_act(reinterpret_cast<float *>(ws + ab), Cin, H, W);
  Act ag = make_act(reinterpret_cast<float *>(ws + 2 * ab), Cout, H, W);
  float *wpk_t = reinterpret_cast<float *>(ws + 2 * ab + gb);
  float *wino_t = wpk_t + conv_wpk_elems(Cout, Cin);
  float *zero_b = wino_t + conv_wino_elems(Cout, Cin);
  float *dw = zero_b + conv_coutp(Cin);
  float *db = dw + conv_wpk_elems(Cin, Cout);
  float *part = db + conv_coutp(Cout);
  float *wt = part + conv_wgrad_part_elems(Cin, Cout, H, W);     // W' in Torch layout (last: its size is no multiple of a record)
  int rc = MPN_OK;
  if (d_grad_in) {
    rc = pack_conv_weights_dgrad(d_w, Cin, Cout, wt, wpk_t, zero_b, dgrad_has_wino(Cout) ? wino_t : nullptr, s);
    if (rc) return rc;
  }
  // the halos of all three maps (the convolutions' padding) and their pad channels: zeroed here, whatever the workspace held
  MPN_CHECK_HIP(hipMemsetAsync(ws, 0, 2 * ab + gb, s));
  for (int b = 0; b < B; ++b) {
    rc = nchw_to_c8p(d_grad_out + (size_t)b * Cout * H * W, Cout, H, W, ag, s);
    if (rc) return rc;
    if (d_grad_b) { rc = conv_bias_grad(ag, db, b > 0, s); if (rc) return rc; }
    if (d_grad_w) {
      rc = nchw_to_c8p(d_in + (size_t)b * Cin * H * W, Cin, H, W, ax, s);
      if (rc == MPN_OK) rc = conv3x3_wgrad(ax, ag, part, dw, b > 0, s);
      if (rc) return rc;
    }
    if (d_grad_in) {
      rc = conv3x3_c8p(ag, wpk_t, zero_b, Cin, 0, adx, Act{}, s, dgrad_has_wino(Cout) ? wino_t : nullptr);
      if (rc == MPN_OK) rc = c8p_to_nchw(adx, d_grad_in + (size_t)b * Cin * H * W, s);
      if (rc) return rc;
    }
  }
  if (d_grad_w) { rc = unpack_conv_weights(dw, nullptr, Cin, Cout, d_grad_w, nullptr, s); if (rc) return rc; }
  if (d_grad_b) MPN_CHECK_HIP(hipMemcpyAsync(d_grad_b, db, (size_t)Cout * sizeof(float), hipMemcpyDeviceToDevice, s));
  return MPN_OK;
}
