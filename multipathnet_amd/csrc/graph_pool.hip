// graph_pool.hip — the graph executor's pooling side: max / average / ROI / global-average pooling, LRN, the image transform, the
// sortable-bf16 map and its range-max tables, the C8I <-> C8P and pixel-major conversions, and the host functions that pick a form
// and launch it.
#include "graph_internal.h"

namespace mpn {

// nn.SpatialMaxPooling(k,k,s,s,p,p), floor mode, on C8I
__global__ void maxpool2d_c8i_kernel(const float *__restrict__ in, int Cb, int B, int H, int W, size_t pitch_in, int k, int stride, int pad, int OH,
                                     int OW, size_t pitch_out, float *__restrict__ out) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)Cb * B * OH * OW * 2;
  if (t >= total) return;
  const int h = (int)(t & 1); size_t r = t >> 1;
  const int ox = (int)(r % OW); r /= OW;
  const int oy = (int)(r % OH); r /= OH;
  const int b = (int)(r % B); const size_t cb = r / B;
  f32x4 m = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int ky = 0; ky < k; ++ky)
    for (int kx = 0; kx < k; ++kx) {
      const int iy = oy * stride + ky - pad, ix = ox * stride + kx - pad;
      if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
      const f32x4 v = *reinterpret_cast<const f32x4 *>(in + (cb * pitch_in + ((size_t)b * H + iy) * W + ix) * 8 + h * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] = v[e] > m[e] ? v[e] : m[e];
    }
  *reinterpret_cast<f32x4 *>(out + (cb * pitch_out + ((size_t)b * OH + oy) * OW + ox) * 8 + h * 4) = m;
}

// image transformer (modules/ImageTransformer.lua:19-33, f64 arithmetic) into a one-map C8I image (channels 3..7 zero)
__global__ void image_transform_c8i_kernel(const float *__restrict__ in, int H, int W, int s0, int s1, int s2, double scale, double m0,
                                           double m1, double m2, double d0, double d1, double d2, int has_std, float *__restrict__ out,
                                           float *__restrict__ planar) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t plane = (size_t)H * W;
  if (t >= plane) return;
  double v0 = (double)in[(size_t)s0 * plane + t], v1 = (double)in[(size_t)s1 * plane + t], v2 = (double)in[(size_t)s2 * plane + t];
  if (scale != 1.0) { v0 = v0 * scale; v1 = v1 * scale; v2 = v2 * scale; }
  v0 = v0 + (-m0); v1 = v1 + (-m1); v2 = v2 + (-m2);
  if (has_std) { v0 = v0 / d0; v1 = v1 / d1; v2 = v2 / d2; }
  *reinterpret_cast<f32x4 *>(out + t * 8) = f32x4{(float)v0, (float)v1, (float)v2, 0.0f};
  *reinterpret_cast<f32x4 *>(out + t * 8 + 4) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  if (planar) { planar[t] = (float)v0; planar[plane + t] = (float)v1; planar[2 * plane + t] = (float)v2; }
}

// inn.ROIPooling on a one-map C8I feature -> [N][Cb][PH][PW][8] (the batch the per-ROI head convolves); the bin arithmetic
// is the same as roi_pool_c8_kernel / the oracle's orc_roi_pool (coord_offset 1, end_adjust 0)
__global__ void roi_pool_c8i_kernel(const float *__restrict__ feat, int Cb, int H, int W, size_t pitch_f, const float *__restrict__ rois, int roi_stride,
                                    int N, int PH, int PW, float scale, float *__restrict__ out, size_t pitch_o, int roi_bins) {
  const int PP = PH * PW;
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)N * Cb * PP * 2;
  if (t >= total) return;
  const int h = (int)(t & 1); size_t r = t >> 1;
  const int bin = (int)(r % PP); r /= PP;
  const int cb = (int)(r % Cb); const int n = (int)(r / Cb);
  const int ph = bin / PW, pw = bin - ph * PW;
  const float *ro = rois + (size_t)roi_stride * n;
  int hs, he, ws, we;
  roi_bin_bounds(ro, scale, RoiRule{1.0f, 0, roi_bins}, H, W, PH, PW, ph, pw, hs, he, ws, we);
  const bool empty = (he <= hs) || (we <= ws);
  f32x4 m = empty ? f32x4{0, 0, 0, 0} : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  const float *fp = feat + (size_t)cb * pitch_f * 8 + h * 4;
  for (int y = hs; y < he; ++y)
    for (int x = ws; x < we; ++x) {
      const f32x4 v = *reinterpret_cast<const f32x4 *>(fp + ((size_t)y * W + x) * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] = v[e] > m[e] ? v[e] : m[e];
    }
  *reinterpret_cast<f32x4 *>(out + ((size_t)cb * pitch_o + ((size_t)n * PH + ph) * PW + pw) * 8 + h * 4) = m;
}

// the same pooling with the bin arithmetic done once per (roi, bin): a thread owns one output row for CBG channel blocks, reads
// whole 32-byte records and a wave stores 64 consecutive records (the kernel above spends most of its instructions on the
// per-thread bin arithmetic for 16 output bytes).  Same cells, same comparisons, same order: bit-identical to it.
template <int CBG>
__global__ __launch_bounds__(256) void roi_pool_c8i_rows_kernel(const float *__restrict__ feat, int H, int W, size_t pitch_f, const float *__restrict__ rois,
                                                                 int roi_stride, int N, int PH, int PW, float scale, float *__restrict__ out, size_t pitch_o,
                                                                 int fc_mp, int roi_bins) {
  const int PP = PH * PW;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)N * PP) return;
  const int n = (int)(t / PP), bin = (int)(t - (size_t)n * PP);
  const int ph = bin / PW, pw = bin - ph * PW;
  const float *ro = rois + (size_t)roi_stride * n;
  int hs, he, ws, we;
  roi_bin_bounds(ro, scale, RoiRule{1.0f, 0, roi_bins}, H, W, PH, PW, ph, pw, hs, he, ws, we);
  const bool empty = (he <= hs) || (we <= ws);
  const int cb0 = blockIdx.y * CBG;
  const float *fp = feat + (size_t)cb0 * pitch_f * 8;
  // fc_mp > 0: the (bin, roi)-row C8 matrix [Cb][PP][fc_mp][8] a fully-connected first layer reads as its GEMM operand
  // (plane = (channel block, bin), row = roi — the VGG pipeline's fc6 layout), instead of the C8I batch of maps
  float *op = fc_mp > 0 ? out + (((size_t)cb0 * PP + bin) * fc_mp + n) * 8 : out + ((size_t)cb0 * pitch_o + t) * 8;
  const size_t plane_o = fc_mp > 0 ? (size_t)PP * fc_mp : pitch_o;
  const float lowest = empty ? 0.0f : -INFINITY;
  f32x4 lo[CBG], hi[CBG];
#pragma unroll
  for (int c = 0; c < CBG; ++c) lo[c] = hi[c] = f32x4{lowest, lowest, lowest, lowest};
  for (int y = hs; y < he; ++y)
    for (int x = ws; x < we; ++x) {
      const float *px = fp + ((size_t)y * W + x) * 8;
#pragma unroll
      for (int c = 0; c < CBG; ++c) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(px + (size_t)c * pitch_f * 8), b = *reinterpret_cast<const f32x4 *>(px + (size_t)c * pitch_f * 8 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { lo[c][e] = a[e] > lo[c][e] ? a[e] : lo[c][e]; hi[c][e] = b[e] > hi[c][e] ? b[e] : hi[c][e]; }
      }
    }
#pragma unroll
  for (int c = 0; c < CBG; ++c) {
    *reinterpret_cast<f32x4 *>(op + (size_t)c * plane_o * 8) = lo[c];
    *reinterpret_cast<f32x4 *>(op + (size_t)c * plane_o * 8 + 4) = hi[c];
  }
}

// 7x7 global average pool of [N][Cb][H][W][8] into the C8 matrix [Cb][Mp][8] the head GEMM reads (row = roi); the sum
// runs in row-major order like the oracle's, then * 1/(H*W)
__global__ void avgpool_c8i_to_c8_kernel(const float *__restrict__ in, int N, int Cb, int HW, size_t pitch, float inv, float *__restrict__ out,
                                         int Mp) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)N * Cb * 2;
  if (t >= total) return;
  const int h = (int)(t & 1); size_t r = t >> 1;
  const int n = (int)(r % N); const int cb = (int)(r / N);
  const float *ip = in + ((size_t)cb * pitch + (size_t)n * HW) * 8 + h * 4;
  f32x4 sacc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < HW; ++i) sacc += *reinterpret_cast<const f32x4 *>(ip + (size_t)i * 8);
  *reinterpret_cast<f32x4 *>(out + ((size_t)cb * Mp + n) * 8 + h * 4) = sacc * inv;
}

// one thread = one 16-byte pixel record (8 channels)
__global__ void maxpool2d_c8i_bf16_kernel(const bf16_t *__restrict__ in, int Cb, int B, int H, int W, size_t pitch_in, int k, int stride, int pad,
                                          int OH, int OW, size_t pitch_out, bf16_t *__restrict__ out) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)Cb * B * OH * OW;
  if (t >= total) return;
  size_t r = t;
  const int ox = (int)(r % OW); r /= OW;
  const int oy = (int)(r % OH); r /= OH;
  const int b = (int)(r % B); const size_t cb = r / B;
  float m[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
  const u32x4 *ip = reinterpret_cast<const u32x4 *>(in) + cb * pitch_in + (size_t)b * H * W;
  for (int ky = 0; ky < k; ++ky)
    for (int kx = 0; kx < k; ++kx) {
      const int iy = oy * stride + ky - pad, ix = ox * stride + kx - pad;
      if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
      const u32x4 v = ip[(size_t)iy * W + ix];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned w = v[e];
        const float lo = __uint_as_float(w << 16), hi = __uint_as_float(w & 0xffff0000u);
        m[2 * e] = lo > m[2 * e] ? lo : m[2 * e];
        m[2 * e + 1] = hi > m[2 * e + 1] ? hi : m[2 * e + 1];
      }
    }
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(m[2 * e], m[2 * e + 1]);
  reinterpret_cast<u32x4 *>(out)[cb * pitch_out + ((size_t)b * OH + oy) * OW + ox] = o;
}

// transformed image as bf16 C8I with TWO channel-block planes (channels 3..15 zero: the MFMA consumes chunk pairs)
__global__ void image_transform_c8i_bf16_kernel(const float *__restrict__ in, int H, int W, int s0, int s1, int s2, double scale, double m0,
                                                double m1, double m2, double d0, double d1, double d2, int has_std, bf16_t *__restrict__ out,
                                                size_t pitch) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t plane = (size_t)H * W;
  if (t >= plane) return;
  double v0 = (double)in[(size_t)s0 * plane + t], v1 = (double)in[(size_t)s1 * plane + t], v2 = (double)in[(size_t)s2 * plane + t];
  if (scale != 1.0) { v0 = v0 * scale; v1 = v1 * scale; v2 = v2 * scale; }
  v0 = v0 + (-m0); v1 = v1 + (-m1); v2 = v2 + (-m2);
  if (has_std) { v0 = v0 / d0; v1 = v1 / d1; v2 = v2 / d2; }
  u16x4 lo = {f2bf((float)v0), f2bf((float)v1), f2bf((float)v2), 0}, z = {0, 0, 0, 0};
  *reinterpret_cast<u16x4 *>(out + t * 8) = lo;
  *reinterpret_cast<u16x4 *>(out + t * 8 + 4) = z;
  *reinterpret_cast<u16x4 *>(out + (pitch + t) * 8) = z;
  *reinterpret_cast<u16x4 *>(out + (pitch + t) * 8 + 4) = z;
}

__global__ void roi_pool_c8i_bf16_kernel(const bf16_t *__restrict__ feat, int Cb, int H, int W, size_t pitch_f, const float *__restrict__ rois,
                                         int roi_stride, int N, int PH, int PW, float scale, bf16_t *__restrict__ out, size_t pitch_o, int roi_bins) {
  const int PP = PH * PW;
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)N * Cb * PP * 2;
  if (t >= total) return;
  const int h = (int)(t & 1); size_t r = t >> 1;
  const int bin = (int)(r % PP); r /= PP;
  const int cb = (int)(r % Cb); const int n = (int)(r / Cb);
  const int ph = bin / PW, pw = bin - ph * PW;
  const float *ro = rois + (size_t)roi_stride * n;
  int hs, he, ws, we;
  roi_bin_bounds(ro, scale, RoiRule{1.0f, 0, roi_bins}, H, W, PH, PW, ph, pw, hs, he, ws, we);
  const bool empty = (he <= hs) || (we <= ws);
  f32x4 m = empty ? f32x4{0, 0, 0, 0} : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  const bf16_t *fp = feat + (size_t)cb * pitch_f * 8 + h * 4;
  for (int y = hs; y < he; ++y)
    for (int x = ws; x < we; ++x) {
      const u16x4 v = *reinterpret_cast<const u16x4 *>(fp + ((size_t)y * W + x) * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float f = bf2f(v[e]); m[e] = f > m[e] ? f : m[e]; }
    }
  u16x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = f2bf(m[e]);
  *reinterpret_cast<u16x4 *>(out + ((size_t)cb * pitch_o + ((size_t)n * PH + ph) * PW + pw) * 8 + h * 4) = o;
}

// ---- ROI max-pooling, bf16, fast path ---------------------------------------------------------------------------------------
// The kernel above spends ~200 instructions per 8 output bytes (per-thread bin arithmetic, 4 channels per thread).  Here the
// feature map is first re-coded so that bf16 order is int16 order (negative values: magnitude bits flipped — a monotone,
// self-inverse map, so max commutes with it), and a thread owns one (roi, bin) for a run of
// channel blocks: the bin arithmetic is done once, each pixel record (8 channels) costs one 16-byte load + 4 v_pk_max_i16, and a
// wave's stores are 64 consecutive records.  Against roi_pool_c8i_bf16_kernel's `f > m` the result is the same VALUE everywhere and the same
// bits except the sign of a zero: a window whose maximum is zero and that holds both zeros gives +0 here (code 0 > code -1) and the zero met
// first there.  NaNs: the encoder below gives a NaN of either sign -inf's code, so — as `f > m` from -inf does — the maxima ignore the NaNs of
// a window and a window of NaNs alone gives -inf (include/mpn.h); the raw order would have put +NaN above +inf.
typedef short i16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned bf16x2_sortable(unsigned x) { return x ^ (((x >> 15) & 0x00010001u) * 0x7fffu); }

__device__ __forceinline__ unsigned bf16x2_sortable_enc(unsigned x) {  // bf16x2_sortable, NaN -> the code of -inf (0x807f)
  unsigned c = bf16x2_sortable(x);
  if ((x & 0x00007fffu) > 0x00007f80u) c = (c & 0xffff0000u) | 0x0000807fu;
  if ((x & 0x7fff0000u) > 0x7f800000u) c = (c & 0x0000ffffu) | 0x807f0000u;
  return c;
}

__global__ void bf16_sortable_kernel(const u32x4 *__restrict__ in, size_t n, u32x4 *__restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  u32x4 v = in[t];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = bf16x2_sortable_enc(v[e]);
  out[t] = v;
}

// vertical range-max (sparse) table level of the sortable map: out[y] = max(prev[y], prev[y + step]) = max over rows y .. y + 2 * step - 1
// (rows past H - 2 * step are never queried).  The fused ROI max-pool below then reads two rows per window column instead of all of them.
__global__ void vmax_level_sorted_kernel(const u32x4 *__restrict__ prev, u32x4 *__restrict__ out, int H, int W, size_t pitch, int Cb, int step) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t HW = (size_t)H * W;
  if (t >= HW * Cb) return;
  const int cb = (int)(t / HW); const size_t px = t - (size_t)cb * HW;
  const int y = (int)(px / W);
  const u32x4 a = prev[(size_t)cb * pitch + px];
  const u32x4 b = prev[(size_t)cb * pitch + px + (y + step < H ? (size_t)step * W : 0)];
  u32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const unsigned ua = a[e], ub = b[e];
    const i16x2 mx = __builtin_elementwise_max(__builtin_bit_cast(i16x2, ua), __builtin_bit_cast(i16x2, ub));
    r[e] = __builtin_bit_cast(unsigned, mx);
  }
  out[(size_t)cb * pitch + px] = r;
}

template <int CBG, bool NT = false>  // channel blocks per thread (grid.y = Cb / CBG); NT: non-temporal stores (timing experiment, debug flavour)
__global__ __launch_bounds__(256) void roi_pool_c8i_bf16_sorted_kernel(const u32x4 *__restrict__ feat, int H, int W, size_t pitch_f,
                                                                        const float *__restrict__ rois, int roi_stride, int N, int PH, int PW, float scale,
                                                                        u32x4 *__restrict__ out, size_t pitch_o, int roi_bins) {
  const int PP = PH * PW;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // (roi, bin): the output row of the pooled batch
  if (t >= (size_t)N * PP) return;
  const int n = (int)(t / PP), bin = (int)(t - (size_t)n * PP);
  const int ph = bin / PW, pw = bin - ph * PW;
  const float *ro = rois + (size_t)roi_stride * n;
  int hs, he, ws, we;
  roi_bin_bounds(ro, scale, RoiRule{1.0f, 0, roi_bins}, H, W, PH, PW, ph, pw, hs, he, ws, we);
  const bool empty = (he <= hs) || (we <= ws);
  const int cb0 = blockIdx.y * CBG;
  const u32x4 *fp = feat + (size_t)cb0 * pitch_f;
  u32x4 *op = out + (size_t)cb0 * pitch_o + t;
  const unsigned lowest = 0x80008000u;  // int16 minimum in both halves
  u32x4 m[CBG];
#pragma unroll
  for (int c = 0; c < CBG; ++c) m[c] = u32x4{lowest, lowest, lowest, lowest};
  for (int y = hs; y < he; ++y)
    for (int x = ws; x < we; ++x) {
      const size_t px = (size_t)y * W + x;
#pragma unroll
      for (int c = 0; c < CBG; ++c) {
        const u32x4 v = fp[(size_t)c * pitch_f + px];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const unsigned cur = m[c][e], val = v[e];  // scalar copies: __builtin_bit_cast of a vector-element lvalue reads element 0
          const i16x2 mx = __builtin_elementwise_max(__builtin_bit_cast(i16x2, cur), __builtin_bit_cast(i16x2, val));
          m[c][e] = __builtin_bit_cast(unsigned, mx);
        }
      }
    }
#pragma unroll
  for (int c = 0; c < CBG; ++c) {
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = empty ? 0u : bf16x2_sortable(m[c][e]);
    if constexpr (NT) __builtin_nontemporal_store(o, &op[(size_t)c * pitch_o]);
    else op[(size_t)c * pitch_o] = o;
  }
}

// max-pool OF the ROI-pooled map, straight from the feature map (graph heads: Inception's Mixed_7a pools its input — the ROI-pooled
// 17 x 17 x 768 tensor, 0.9 GB for 2000 ROIs — 3 x 3 / 2; max of maxes = one max over the union of the bins' windows).  Output pixel
// (oy, ox) covers bins [o * stride - pad, + k) clipped to the bin grid; consecutive bins touch or overlap (ceil((b + 1) h) >= floor((b + 1) h)),
// so the union of their windows is ONE window of the map; a bin that falls outside the map is empty and holds 0 in the pooled tensor, so 0
// joins the max when the group has one.  Bin bounds are the pooling kernel's own expressions; max is exact: the result is the two-step
// result bit for bit (up to the sign of a zero), and the max-pool launch that re-read the pooled tensor (210 us, 5.2 TB/s) is gone.
template <int CBG>
__global__ __launch_bounds__(256) void roi_maxpool_c8i_bf16_sorted_kernel(const u32x4 *__restrict__ feat, int H, int W, size_t pitch_f,
                                                                           const float *__restrict__ rois, int roi_stride, int N, int PH, int PW, float scale,
                                                                           int k, int stride, int pad, int OH, int OW, u32x4 *__restrict__ out, size_t pitch_o,
                                                                           const u32x4 *__restrict__ tabs, size_t level_elems, int n_levels) {
  const int OP = OH * OW;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // (roi, output pixel): the output row of the max-pooled batch
  if (t >= (size_t)N * OP) return;
  const int n = (int)(t / OP), o = (int)(t - (size_t)n * OP);
  const int oy = o / OW, ox = o - oy * OW;
  const float *ro = rois + (size_t)roi_stride * n;
  const int sw = (int)roundf((ro[1] - 1.0f) * scale), sh = (int)roundf((ro[2] - 1.0f) * scale);
  const int ew = (int)roundf((ro[3] - 1.0f) * scale), eh = (int)roundf((ro[4] - 1.0f) * scale);
  const int rw = max(ew - sw + 1, 1), rh = max(eh - sh + 1, 1);
  const float bh = (float)rh / (float)PH, bw = (float)rw / (float)PW;
  bool any_empty = false;
  int hs = 0x7fffffff, he = -1, ws = 0x7fffffff, we = -1;
  for (int ph = max(oy * stride - pad, 0); ph < min(oy * stride - pad + k, PH); ++ph) {
    int a = (int)floorf((float)ph * bh) + sh, b = (int)ceilf((float)(ph + 1) * bh) + sh;
    a = min(max(a, 0), H); b = min(max(b, 0), H);
    if (b <= a) any_empty = true; else { hs = min(hs, a); he = max(he, b); }
  }
  for (int pw = max(ox * stride - pad, 0); pw < min(ox * stride - pad + k, PW); ++pw) {
    int a = (int)floorf((float)pw * bw) + sw, b = (int)ceilf((float)(pw + 1) * bw) + sw;
    a = min(max(a, 0), W); b = min(max(b, 0), W);
    if (b <= a) any_empty = true; else { ws = min(ws, a); we = max(we, b); }
  }
  const int cb0 = blockIdx.y * CBG;
  const u32x4 *fp = feat + (size_t)cb0 * pitch_f;
  u32x4 *op = out + (size_t)cb0 * pitch_o + t;
  const unsigned lowest = 0x80008000u;  // int16 minimum in both halves
  u32x4 m[CBG];
#pragma unroll
  for (int c = 0; c < CBG; ++c) m[c] = u32x4{lowest, lowest, lowest, lowest};
  // rows [hs, he) as ceil(h / 2^lv) blocks of 2^lv rows from table level lv (the last block pulled back to end at he: overlap is
  // harmless for a max); lv = floor(log2 h) capped at the levels built -> two row reads per column for any window height
  int lv = 0, bstep = 1;
  if (tabs && he - hs > 1) {
    lv = min(31 - __builtin_clz((unsigned)(he - hs)), n_levels);
    bstep = 1 << lv;
    if (lv > 0) fp = tabs + (size_t)(lv - 1) * level_elems + (size_t)cb0 * pitch_f;
  }
  for (int y0 = hs; y0 < he; y0 += bstep) {
    const int y = min(y0, he - bstep);
    for (int x = ws; x < we; ++x) {
      const size_t px = (size_t)y * W + x;
#pragma unroll
      for (int c = 0; c < CBG; ++c) {
        const u32x4 v = fp[(size_t)c * pitch_f + px];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const unsigned cur = m[c][e], val = v[e];
          const i16x2 mx = __builtin_elementwise_max(__builtin_bit_cast(i16x2, cur), __builtin_bit_cast(i16x2, val));
          m[c][e] = __builtin_bit_cast(unsigned, mx);
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < CBG; ++c) {
    u32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      unsigned cur = m[c][e];
      if (any_empty) {  // an empty bin's 0.0 (sortable code 0) takes part in the max
        const i16x2 mx = __builtin_elementwise_max(__builtin_bit_cast(i16x2, cur), i16x2{0, 0});
        cur = __builtin_bit_cast(unsigned, mx);
      }
      r[e] = bf16x2_sortable(cur);
    }
    op[(size_t)c * pitch_o] = r;
  }
}

// average pool of the bf16 maps into the fp32 C8 matrix the (fp32) head GEMM reads.  Block = one channel block x 16 maps: the
// 16 * HW records are read as consecutive 16-byte loads (fully coalesced) into LDS as fp32, then 128 threads (map, channel) sum
// their HW values in pixel order (the order of the plain kernel below, so the result is bit-identical to it).
__global__ __launch_bounds__(256) void avgpool_c8i_bf16_to_c8_lds_kernel(const bf16_t *__restrict__ in, int N, int HW, size_t pitch, float inv,
                                                                          float *__restrict__ out, int Mp) {
  extern __shared__ float sm[];  // [16 * HW][8 + 1]: odd row stride -> the 128 summing threads hit distinct banks
  const int cb = blockIdx.y, n0 = blockIdx.x * 16;
  const int nm = min(16, N - n0);
  const int nrec = nm * HW;
  const u32x4 *src = reinterpret_cast<const u32x4 *>(in) + (size_t)cb * pitch + (size_t)n0 * HW;
  for (int i = threadIdx.x; i < nrec; i += 256) {
    const u32x4 v = src[i];
    float *d = sm + i * 9;
#pragma unroll
    for (int e = 0; e < 4; ++e) { d[2 * e] = __uint_as_float(v[e] << 16); d[2 * e + 1] = __uint_as_float(v[e] & 0xffff0000u); }
  }
  __syncthreads();
  const int m = threadIdx.x >> 3, c = threadIdx.x & 7;
  if (threadIdx.x < 128 && m < nm) {
    const float *d = sm + (size_t)m * HW * 9 + c;
    float acc = 0.0f;
    for (int i = 0; i < HW; ++i) acc += d[i * 9];
    out[((size_t)cb * Mp + n0 + m) * 8 + c] = acc * inv;
  }
}


__global__ void avgpool_c8i_bf16_to_c8_kernel(const bf16_t *__restrict__ in, int N, int Cb, int HW, size_t pitch, float inv, float *__restrict__ out,
                                              int Mp) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)N * Cb * 2;
  if (t >= total) return;
  const int h = (int)(t & 1); size_t r = t >> 1;
  const int n = (int)(r % N); const int cb = (int)(r / N);
  const bf16_t *ip = in + ((size_t)cb * pitch + (size_t)n * HW) * 8 + h * 4;
  f32x4 sacc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < HW; ++i) {
    const u16x4 v = *reinterpret_cast<const u16x4 *>(ip + (size_t)i * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) sacc[e] += bf2f(v[e]);
  }
  *reinterpret_cast<f32x4 *>(out + ((size_t)cb * Mp + n) * 8 + h * 4) = sacc * inv;
}

// nn.SpatialAveragePooling(kw,kh,sw,sh,pw,ph), count_include_pad (torch's default): sum over the in-map cells of the window
// in row-major order, divided by kh*kw regardless of how many cells lie in the padding.  T = float or bf16_t.
template <typename T>
__global__ void avgpool2d_c8i_kernel(const T *__restrict__ in, int Cb, int B, int H, int W, size_t pitch_in, int kh, int kw, int sh, int sw, int ph,
                                     int pw, int OH, int OW, size_t pitch_out, T *__restrict__ out, const float *__restrict__ bias, int relu) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)Cb * B * OH * OW * 2;
  if (t >= total) return;
  const int h = (int)(t & 1); size_t r = t >> 1;
  const int ox = (int)(r % OW); r /= OW;
  const int oy = (int)(r % OH); r /= OH;
  const int b = (int)(r % B); const size_t cb = r / B;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ky = 0; ky < kh; ++ky)
    for (int kx = 0; kx < kw; ++kx) {
      const int iy = oy * sh + ky - ph, ix = ox * sw + kx - pw;
      if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
      const size_t off = (cb * pitch_in + ((size_t)b * H + iy) * W + ix) * 8 + h * 4;
      if constexpr (sizeof(T) == 2) {
        const u16x4 v = *reinterpret_cast<const u16x4 *>(in + off);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += bf2f(v[e]);
      } else {
        acc += *reinterpret_cast<const f32x4 *>(in + off);
      }
    }
  const float inv = 1.0f / (float)(kh * kw);
  const size_t oo = (cb * pitch_out + ((size_t)b * OH + oy) * OW + ox) * 8 + h * 4;
  acc = acc * inv;
  if (bias) {  // a commuted pool -> pointwise-convolution pair (graph_parse): the convolution's bias and ReLU follow the pool
#pragma unroll
    for (int e = 0; e < 4; ++e) { acc[e] += bias[cb * 8 + h * 4 + e]; if (relu && acc[e] < 0.0f) acc[e] = 0.0f; }
  }
  if constexpr (sizeof(T) == 2) {
    u16x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = f2bf(acc[e]);
    *reinterpret_cast<u16x4 *>(out + oo) = o;
  } else {
    *reinterpret_cast<f32x4 *>(out + oo) = acc;
  }
}

// bf16: one thread = one 16-byte pixel record; same summation order per channel as the template above
__global__ void avgpool2d_c8i_bf16_kernel(const bf16_t *__restrict__ in, int Cb, int B, int H, int W, size_t pitch_in, int kh, int kw, int sh, int sw,
                                          int ph, int pw, int OH, int OW, size_t pitch_out, bf16_t *__restrict__ out, const float *__restrict__ bias, int relu) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)Cb * B * OH * OW;
  if (t >= total) return;
  size_t r = t;
  const int ox = (int)(r % OW); r /= OW;
  const int oy = (int)(r % OH); r /= OH;
  const int b = (int)(r % B); const size_t cb = r / B;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
  const u32x4 *ip = reinterpret_cast<const u32x4 *>(in) + cb * pitch_in + (size_t)b * H * W;
  for (int ky = 0; ky < kh; ++ky)
    for (int kx = 0; kx < kw; ++kx) {
      const int iy = oy * sh + ky - ph, ix = ox * sw + kx - pw;
      if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
      const u32x4 v = ip[(size_t)iy * W + ix];
#pragma unroll
      for (int e = 0; e < 4; ++e) { acc[2 * e] += __uint_as_float(v[e] << 16); acc[2 * e + 1] += __uint_as_float(v[e] & 0xffff0000u); }
    }
  const float inv = 1.0f / (float)(kh * kw);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    acc[e] *= inv;
    if (bias) { acc[e] += bias[cb * 8 + e]; if (relu && acc[e] < 0.0f) acc[e] = 0.0f; }
  }
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(acc[2 * e], acc[2 * e + 1]);
  reinterpret_cast<u32x4 *>(out)[cb * pitch_out + ((size_t)b * OH + oy) * OW + ox] = o;
}

// stride-1 average pooling of SMALL maps (per-ROI 8x8 in Inception's Mixed_7b/7c: H*W <= 256) through LDS: a block owns
// 256 / (H*W) consecutive maps of one channel block, reads their records once (consecutive 16-byte loads) and takes the window
// cells from LDS — the plain kernel issues kh*kw global loads per output.  Same cells, same order: bit-identical to it.
__global__ __launch_bounds__(256) void avgpool2d_c8i_bf16_small_kernel(const bf16_t *__restrict__ in, int B, int H, int W, size_t pitch_in, int kh, int kw,
                                                                        int ph, int pw, size_t pitch_out, bf16_t *__restrict__ out,
                                                                        const float *__restrict__ bias, int relu) {
  __shared__ u32x4 tile[256];
  const int HW = H * W, mpb = 256 / HW;           // maps per block
  const int cb = blockIdx.y;
  const int b0 = blockIdx.x * mpb;
  const int nrec = min(mpb, B - b0) * HW;
  const int t = threadIdx.x;
  const u32x4 *ip = reinterpret_cast<const u32x4 *>(in) + (size_t)cb * pitch_in + (size_t)b0 * HW;
  if (t < nrec) tile[t] = ip[t];
  __syncthreads();
  if (t >= nrec) return;
  const int m = t / HW, r = t - m * HW;
  const int oy = r / W, ox = r - oy * W;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
  for (int ky = 0; ky < kh; ++ky)
    for (int kx = 0; kx < kw; ++kx) {
      const int iy = oy + ky - ph, ix = ox + kx - pw;
      if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
      const u32x4 v = tile[m * HW + iy * W + ix];
#pragma unroll
      for (int e = 0; e < 4; ++e) { acc[2 * e] += __uint_as_float(v[e] << 16); acc[2 * e + 1] += __uint_as_float(v[e] & 0xffff0000u); }
    }
  const float inv = 1.0f / (float)(kh * kw);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    acc[e] *= inv;
    if (bias) { acc[e] += bias[cb * 8 + e]; if (relu && acc[e] < 0.0f) acc[e] = 0.0f; }
  }
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(acc[2 * e], acc[2 * e + 1]);
  reinterpret_cast<u32x4 *>(out)[(size_t)cb * pitch_out + (size_t)b0 * HW + t] = o;
}

// ------------------------------------------------------------------------------------------------------------------------
// graph
// ------------------------------------------------------------------------------------------------------------------------
// nn.SpatialCrossMapLRN(size, alpha, beta, k) on C8I (models/alexnet.lua's trunk: norm1 / norm2): one thread per (pixel row, channel
// block); the window spans at most one block either side (size <= 17).  fp32, squares summed in ascending channel order.
__global__ void lrn_c8i_kernel(const float *__restrict__ in, int Cb, int C, size_t rows, size_t pitch_in, int size, float alpha, float beta, float k,
                               size_t pitch_out, float *__restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * Cb) return;
  const size_t row = t % rows;
  const int cb = (int)(t / rows);
  float v[24];  // channels 8*cb - 8 .. 8*cb + 15
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int b = cb - 1 + q;
    f32x4 lo = f32x4{0, 0, 0, 0}, hi = lo;
    if (b >= 0 && b < Cb) {
      const float *p = in + ((size_t)b * pitch_in + row) * 8;
      lo = *reinterpret_cast<const f32x4 *>(p); hi = *reinterpret_cast<const f32x4 *>(p + 4);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[q * 8 + e] = lo[e]; v[q * 8 + 4 + e] = hi[e]; }
  }
  const int half = (size - 1) / 2;
  const float a = alpha / (float)size;
  float o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = cb * 8 + j;
    float ssum = 0.0f;
#pragma unroll
    for (int d = -8; d <= 8; ++d) {  // static register indices; the window is [-half, half]
      const int cc = c + d;
      if (d >= -half && d <= half && cc >= 0 && cc < C) { const float x = v[8 + j + d]; ssum = ssum + x * x; }
    }
    const float sc = k + a * ssum;
    o[j] = c < C ? v[8 + j] * powf(sc, -beta) : 0.0f;
  }
  float *q = out + ((size_t)cb * pitch_out + row) * 8;
  *reinterpret_cast<f32x4 *>(q) = f32x4{o[0], o[1], o[2], o[3]};
  *reinterpret_cast<f32x4 *>(q + 4) = f32x4{o[4], o[5], o[6], o[7]};
}

// C8I map (B = 1) <-> C8P map (dense.h: one zero halo row / column in front, padded behind): the trunk's 3x3 / stride-1 / pad-1
// convolutions run on dense.hip's Winograd F(2x2,3x3) kernel, which reads its halo tiles straight from the padded layout
__global__ void c8i_to_c8p_kernel(const float *__restrict__ in, int Cb, int H, int W, size_t pitch, int Hp, int Wp, float *__restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t HW = (size_t)H * W;
  if (t >= HW * Cb * 2) return;
  const int h = (int)(t & 1); size_t r = t >> 1;
  const size_t px = r % HW; const int cb = (int)(r / HW);
  const int y = (int)(px / W), x = (int)(px - (size_t)y * W);
  *reinterpret_cast<f32x4 *>(out + (((size_t)cb * Hp + y + 1) * Wp + x + 1) * 8 + h * 4) = *reinterpret_cast<const f32x4 *>(in + ((size_t)cb * pitch + px) * 8 + h * 4);
}
__global__ void c8p_to_c8i_kernel(const float *__restrict__ in, int Cb, int H, int W, int Hp, int Wp, size_t pitch, float *__restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t HW = (size_t)H * W;
  if (t >= HW * Cb * 2) return;
  const int h = (int)(t & 1); size_t r = t >> 1;
  const size_t px = r % HW; const int cb = (int)(r / HW);
  const int y = (int)(px / W), x = (int)(px - (size_t)y * W);
  *reinterpret_cast<f32x4 *>(out + ((size_t)cb * pitch + px) * 8 + h * 4) = *reinterpret_cast<const f32x4 *>(in + (((size_t)cb * Hp + y + 1) * Wp + x + 1) * 8 + h * 4);
}

// one-map C8I -> pixel-major [y][x][Cb * 8] (dense.h roi_pool_pm's operand: a pixel's channels contiguous)
__global__ void c8i_to_pixel_major_kernel(const float *__restrict__ in, int Cb, size_t HW, size_t pitch, float *__restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= HW * Cb * 2) return;
  const int q = (int)(t % (Cb * 2)); const size_t px = t / (Cb * 2);   // q = cb * 2 + half: consecutive lanes write consecutive 16 bytes
  *reinterpret_cast<f32x4 *>(out + px * (size_t)Cb * 8 + q * 4) = *reinterpret_cast<const f32x4 *>(in + ((size_t)(q >> 1) * pitch + px) * 8 + (q & 1) * 4);
}

MPN_KNOB(int, g_bf16_fast_pool, 3);       // bit 0: row-per-thread ROI pooling (bf16: on the int16-sortable map), bit 1: LDS average pooling (bf16) (0 = the plain kernels; mpn_debug_set_bf16_fast_pool)
#ifdef MPN_DEBUG_HOOKS
static int g_pool_exp = 0;   // mpn_debug_set_pool_exp: timing experiments of the bf16 ROI pooling launch (roi_pool_experiment)
#endif

// ---- host side: every site picks a PoolKernel, records it (RN_POOL) and launches by switching on it ------------------------------------
bool fast_pool_ok(const ResNetGraph *g) { return (g_bf16_fast_pool & 1) && ((g->feat_c + 7) / 8) % 4 == 0; }
// max-pools of the pooled input: from the map (its kernel unions the CUDA branch's bins: the adaptive rule runs the max-pool as an ordinary op on the pooled batch)
bool roi_maxpool_fused(const ResNetGraph *g) { return g->is_graph && g->bf16 && fast_pool_ok(g) && (g_graph_fuse & 4) && g->roi_bins == 0; }

int rn_image_transform(ResNetGraph *g, const float *d_image, int H, int W, const int *swap, double scale, const double *mean, const double *std, int has_std,
                       hipStream_t s) {
  const size_t plane = (size_t)H * W;
  if (g->bf16)
    hipLaunchKernelGGL(image_transform_c8i_bf16_kernel, dim3((unsigned)cdiv_sz(plane, 256)), dim3(256), 0, s, d_image, H, W, swap[0], swap[1], swap[2],
                       scale, mean[0], mean[1], mean[2], has_std ? std[0] : 1.0, has_std ? std[1] : 1.0, has_std ? std[2] : 1.0, has_std,
                       reinterpret_cast<bf16_t *>(g->img), (ActI{g->img, 1, 3, H, W}).pitch());
  else
    hipLaunchKernelGGL(image_transform_c8i_kernel, dim3((unsigned)cdiv_sz(plane, 256)), dim3(256), 0, s, d_image, H, W, swap[0], swap[1], swap[2], scale,
                       mean[0], mean[1], mean[2], has_std ? std[0] : 1.0, has_std ? std[1] : 1.0, has_std ? std[2] : 1.0, has_std, g->img, g->img_planar);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

int rn_stem_maxpool(ResNetGraph *g, const ActI &y, int OH, int OW, hipStream_t s) {
  const size_t total = (size_t)y.Cb() * OH * OW * 2;
  const ActI po{g->tb[1], 1, y.C, OH, OW};
  if (g->bf16)
    hipLaunchKernelGGL(maxpool2d_c8i_bf16_kernel, dim3((unsigned)cdiv_sz(total / 2, 256)), dim3(256), 0, s, reinterpret_cast<const bf16_t *>(y.p), y.Cb(), 1,
                       y.H, y.W, y.pitch(), 3, 2, 1, OH, OW, po.pitch(), reinterpret_cast<bf16_t *>(g->tb[1]));
  else
    hipLaunchKernelGGL(maxpool2d_c8i_kernel, dim3((unsigned)cdiv_sz(total, 256)), dim3(256), 0, s, y.p, y.Cb(), 1, y.H, y.W, y.pitch(), 3, 2, 1, OH, OW,
                       po.pitch(), g->tb[1]);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

int rn_c8i_to_c8p(const GTensor &ps, hipStream_t s) {
  const ActI ti{ps.buf, 1, ps.C, ps.H, ps.W};
  const Act tp = make_act(ps.c8p, ps.C, ps.H, ps.W);
  hipLaunchKernelGGL(c8i_to_c8p_kernel, dim3((unsigned)cdiv_sz((size_t)ps.H * ps.W * ti.Cb() * 2, 256)), dim3(256), 0, s, ps.buf, ti.Cb(), ps.H, ps.W, ti.pitch(),
                     tp.Hp, tp.Wp, ps.c8p);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}
int rn_c8p_to_c8i(const GTensor &t, hipStream_t s) {
  const ActI ti{t.buf, 1, t.C, t.H, t.W};
  const Act tp = make_act(t.c8p, t.C, t.H, t.W);
  hipLaunchKernelGGL(c8p_to_c8i_kernel, dim3((unsigned)cdiv_sz((size_t)t.H * t.W * ti.Cb() * 2, 256)), dim3(256), 0, s, t.c8p, ti.Cb(), t.H, t.W, tp.Hp, tp.Wp,
                     ti.pitch(), t.buf);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// graph_run's max-pool / average-pool / LRN ops; `src` is the op's (channel range of the) source
static PoolKernel pick_pool_op(const ResNetGraph *g, const GOp &op, const GTensor &src, const GTensor &dst) {
  if (op.kind == 3) return PK_LRN;
  if (op.kind == 1) return g->bf16 ? PK_MAX_BF16 : PK_MAX_F32;
  if (g->bf16 && op.sh == 1 && op.sw == 1 && dst.H == src.H && dst.W == src.W && src.H * src.W <= 256) return PK_AVG_BF16_SMALL;
  return g->bf16 ? PK_AVG_BF16 : PK_AVG_F32;
}
// `in`: src as a batch of B maps; od / outp: the destination batch and the op's plane of it (plane offset = the concat)
int rn_pool_op(const ResNetGraph *g, const GOp &op, const GTensor &src, const ActI &in, const GTensor &dst, const ActI &od, char *outp, int B, hipStream_t s) {
  const size_t total = (size_t)in.Cb() * B * dst.H * dst.W * 2;
  const dim3 grid((unsigned)cdiv_sz(total, 256)), grid16((unsigned)cdiv_sz(total / 2, 256));  // fp32: half records, bf16: whole records per thread
  if (op.kind == 1) MPN_CHECK_ARG(op.kh == op.kw && op.sh == op.sw && op.ph == op.pw);
  const PoolKernel form = pick_pool_op(g, op, src, dst);
  RN_POOL(form);
  switch (form) {
  case PK_LRN: {
    const size_t rows = (size_t)B * src.H * src.W;
    hipLaunchKernelGGL(lrn_c8i_kernel, dim3((unsigned)cdiv_sz(rows * in.Cb(), 256)), dim3(256), 0, s, src.buf, in.Cb(), src.C, rows, in.pitch(), op.kh,
                       op.lrn_alpha, op.lrn_beta, op.lrn_k, od.pitch(), reinterpret_cast<float *>(outp));
    break;
  }
  case PK_MAX_BF16:
    hipLaunchKernelGGL(maxpool2d_c8i_bf16_kernel, grid16, dim3(256), 0, s, reinterpret_cast<const bf16_t *>(src.buf), in.Cb(), B, src.H, src.W, in.pitch(),
                       op.kh, op.sh, op.ph, dst.H, dst.W, od.pitch(), reinterpret_cast<bf16_t *>(outp));
    break;
  case PK_MAX_F32:
    hipLaunchKernelGGL(maxpool2d_c8i_kernel, grid, dim3(256), 0, s, src.buf, in.Cb(), B, src.H, src.W, in.pitch(), op.kh, op.sh, op.ph, dst.H, dst.W,
                       od.pitch(), reinterpret_cast<float *>(outp));
    break;
  case PK_AVG_BF16_SMALL: {
    const int mpb = 256 / (src.H * src.W);
    hipLaunchKernelGGL(avgpool2d_c8i_bf16_small_kernel, dim3((unsigned)((B + mpb - 1) / mpb), (unsigned)in.Cb()), dim3(256), 0, s,
                       reinterpret_cast<const bf16_t *>(src.buf), B, src.H, src.W, in.pitch(), op.kh, op.kw, op.ph, op.pw, od.pitch(),
                       reinterpret_cast<bf16_t *>(outp), op.pool_bias, op.relu);
    break;
  }
  case PK_AVG_BF16:
    hipLaunchKernelGGL(avgpool2d_c8i_bf16_kernel, grid16, dim3(256), 0, s, reinterpret_cast<const bf16_t *>(src.buf), in.Cb(), B, src.H, src.W,
                       in.pitch(), op.kh, op.kw, op.sh, op.sw, op.ph, op.pw, dst.H, dst.W, od.pitch(), reinterpret_cast<bf16_t *>(outp), op.pool_bias, op.relu);
    break;
  default:  // PK_AVG_F32
    hipLaunchKernelGGL((avgpool2d_c8i_kernel<float>), grid, dim3(256), 0, s, src.buf, in.Cb(), B, src.H, src.W, in.pitch(), op.kh, op.kw, op.sh, op.sw,
                       op.ph, op.pw, dst.H, dst.W, od.pitch(), reinterpret_cast<float *>(outp), op.pool_bias, op.relu);
  }
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// the ROI pooling of a head: the first matching line is the form
static PoolKernel pick_roi_pool(const ResNetGraph *g, bool fc_gemm) {
  if (g->bf16 && fast_pool_ok(g)) {
#ifdef MPN_DEBUG_HOOKS
    if (g_tower_knock & 1) return PK_NONE;
    if ((g_pool_exp & 3) && ((g->feat_c + 7) / 8) % 8 == 0) return PK_ROI_SORTED_EXP;
#endif
    return PK_ROI_SORTED;
  }
  if (g->bf16) return PK_ROI_BF16;
  if (fc_gemm && (g_graph_fuse & 256)) return PK_ROI_PM;
  if (fast_pool_ok(g)) return PK_ROI_ROWS4;
  return PK_ROI_F32;
}

#ifdef MPN_DEBUG_HOOKS
// Debug flavour only: PK_ROI_SORTED_EXP, the sorted kernel's launch in the variants of mpn_debug_set_pool_exp (timing experiments): 1 = 8 channel
// blocks per thread / ordinary stores, 2 = 4 blocks / ordinary stores (rounds 3-5), 3 = 8 blocks / non-temporal
static void roi_pool_experiment(const ResNetGraph *g, const float *d_rois, int roi_stride, int N, float spatial_scale, float *pool_dst, size_t pitch_f,
                                size_t pitch_p, hipStream_t s) {
  const int Cb = (g->feat_c + 7) / 8, PH = g->pooled;
  const dim3 g8((unsigned)cdiv_sz((size_t)N * PH * PH, 256), (unsigned)(Cb / 8)), g4((unsigned)cdiv_sz((size_t)N * PH * PH, 256), (unsigned)(Cb / 4));
  auto run = [&](auto *kernel, const dim3 &grid) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, reinterpret_cast<const u32x4 *>(g->feat_sorted), g->feat_h, g->feat_w, pitch_f, d_rois, roi_stride, N, PH, PH,
                       spatial_scale, reinterpret_cast<u32x4 *>(pool_dst), pitch_p, g->roi_bins);
  };
  if ((g_pool_exp & 3) == 1) run(roi_pool_c8i_bf16_sorted_kernel<8, false>, g8);
  else if ((g_pool_exp & 3) == 2) run(roi_pool_c8i_bf16_sorted_kernel<4, false>, g4);   // rounds 3-5: ordinary stores
  else run(roi_pool_c8i_bf16_sorted_kernel<8, true>, g8);
}
#endif

// the fused max-pools of a head's pooled input (GOp::from_rois), from the sortable map and, where heads_prepare_impl built them, its range-max tables
static int roi_maxpools_from_map(ResNetGraph *g, int head, std::vector<GTensor> &t_head, const float *d_rois, int roi_stride, int N, float spatial_scale,
                                 size_t pitch_f, hipStream_t s) {
  const int Cb = (g->feat_c + 7) / 8, PH = g->pooled;
  const int want_levels = g->feat_vmax_valid ? g->feat_vmax_levels : 0;
  const PoolKernel form = want_levels > 0 ? PK_ROIMAX_SORTED_TABLES : PK_ROIMAX_SORTED;  // one kernel: with / without the tables
  for (const GOp &op : g->g_heads[head]) {
    if (!op.from_rois) continue;
    MPN_CHECK_LAUNCH();
    const GTensor &dst = t_head[op.dst];
    const ActI od{dst.buf, N, dst.C, dst.H, dst.W};
    char *outp = reinterpret_cast<char *>(dst.buf) + (size_t)(op.dst_c_off / 8) * od.pitch() * 8 * sizeof(bf16_t);  // plane offset = the concat
    RN_POOL(form);
    hipLaunchKernelGGL(roi_maxpool_c8i_bf16_sorted_kernel<4>, dim3((unsigned)cdiv_sz((size_t)N * dst.H * dst.W, 256), (unsigned)(Cb / 4)), dim3(256), 0, s,
                       reinterpret_cast<const u32x4 *>(g->feat_sorted), g->feat_h, g->feat_w, pitch_f, d_rois, roi_stride, N, PH, PH, spatial_scale,
                       op.kh, op.sh, op.ph, dst.H, dst.W, reinterpret_cast<u32x4 *>(outp), od.pitch(),
                       form == PK_ROIMAX_SORTED_TABLES ? reinterpret_cast<const u32x4 *>(g->feat_vmax) : nullptr, g->feat_vmax_elems / 8, want_levels);
  }
  return MPN_OK;
}

// rois -> the pooled batch in pool_dst (fc_gemm: the (bin, roi)-row matrix g->fc_x), and with fuse_mp the head's from_rois max-pools beside it
int rn_roi_pool(ResNetGraph *g, int head, std::vector<GTensor> &t_head, float *pool_dst, const float *d_rois, int roi_stride, int N, float spatial_scale,
                bool fc_gemm, bool fuse_mp, hipStream_t s) {
  const int Cb = (g->feat_c + 7) / 8, PH = g->pooled;
  const size_t total = (size_t)N * Cb * PH * PH * 2;
  const ActI fa{g->feat, 1, g->feat_c, g->feat_h, g->feat_w}, pa{pool_dst, N, g->feat_c, PH, PH};
  const PoolKernel form = pick_roi_pool(g, fc_gemm);
  if (g->bf16 && fast_pool_ok(g)) { int rc_prep = heads_prepare_impl(g, head, s); if (rc_prep) return rc_prep; }  // the sortable map (a no-op when resnet_heads_prepare already ran for this image)
  if (form != PK_NONE) RN_POOL(form);
  switch (form) {
  case PK_NONE: break;  // (debug flavour: knock-out bit 0 launches nothing)
#ifdef MPN_DEBUG_HOOKS
  case PK_ROI_SORTED_EXP: roi_pool_experiment(g, d_rois, roi_stride, N, spatial_scale, pool_dst, fa.pitch(), pa.pitch(), s); break;
#endif
  case PK_ROI_SORTED:
    // non-temporal stores: the 0.4-0.9 GB pooled tensor streams past the L2 instead of evicting the sorted map the launch gathers from
    // (measured, profiles/r06_pool_exp.txt: configs[4] 24.28 -> 24.10 ms, configs[3] bf16 11.06 -> 10.99; 8 channel blocks per thread: slower)
    hipLaunchKernelGGL((roi_pool_c8i_bf16_sorted_kernel<4, true>), dim3((unsigned)cdiv_sz((size_t)N * PH * PH, 256), (unsigned)(Cb / 4)), dim3(256), 0, s,
                       reinterpret_cast<const u32x4 *>(g->feat_sorted), g->feat_h, g->feat_w, fa.pitch(), d_rois, roi_stride, N, PH, PH, spatial_scale,
                       reinterpret_cast<u32x4 *>(pool_dst), pa.pitch(), g->roi_bins);
    break;
  case PK_ROI_BF16:
    hipLaunchKernelGGL(roi_pool_c8i_bf16_kernel, dim3((unsigned)cdiv_sz(total, 256)), dim3(256), 0, s, reinterpret_cast<const bf16_t *>(g->feat), Cb, g->feat_h,
                       g->feat_w, fa.pitch(), d_rois, roi_stride, N, PH, PH, spatial_scale, reinterpret_cast<bf16_t *>(pool_dst), pa.pitch(), g->roi_bins);
    break;
  case PK_ROI_PM: {
    // the fully-connected operand is the VGG pipeline's (bin, roi)-row matrix: its pooling kernel too (a wave = one (roi, bin) over 256
    // channels of a pixel-major copy of the map, four ROIs per block leaving as whole 128-byte lines) — 37 -> 12 us on AlexNet
    void *pm = nullptr;
    { int rc_ws = scratch_get(SCR_MISC, (size_t)g->feat_h * g->feat_w * Cb * 8 * sizeof(float), s, &pm); if (rc_ws) return rc_ws; }
    hipLaunchKernelGGL(c8i_to_pixel_major_kernel, dim3((unsigned)cdiv_sz((size_t)g->feat_h * g->feat_w * Cb * 2, 256)), dim3(256), 0, s, g->feat, Cb,
                       (size_t)g->feat_h * g->feat_w, fa.pitch(), static_cast<float *>(pm));
    MPN_CHECK_LAUNCH();
    const Act fdim{nullptr, g->feat_c, g->feat_h, g->feat_w, 0, 0};
    int rcp = roi_pool_pm(fdim, static_cast<const float *>(pm), d_rois, N, PH, PH, spatial_scale, RoiRule{1.0f, 0, g->roi_bins}, g->fc_x, s, roi_stride, round_up(N, 128));
    if (rcp) return rcp;
    break;
  }
  case PK_ROI_ROWS4:
    hipLaunchKernelGGL(roi_pool_c8i_rows_kernel<4>, dim3((unsigned)cdiv_sz((size_t)N * PH * PH, 256), (unsigned)(Cb / 4)), dim3(256), 0, s, g->feat, g->feat_h,
                       g->feat_w, fa.pitch(), d_rois, roi_stride, N, PH, PH, spatial_scale, fc_gemm ? g->fc_x : pool_dst, pa.pitch(), fc_gemm ? round_up(N, 128) : 0, g->roi_bins);
    break;
  default:  // PK_ROI_F32
    hipLaunchKernelGGL(roi_pool_c8i_kernel, dim3((unsigned)cdiv_sz(total, 256)), dim3(256), 0, s, g->feat, Cb, g->feat_h, g->feat_w, fa.pitch(), d_rois, roi_stride,
                       N, PH, PH, spatial_scale, pool_dst, pa.pitch(), g->roi_bins);
  }
  if (fuse_mp) { int rc_mp = roi_maxpools_from_map(g, head, t_head, d_rois, roi_stride, N, spatial_scale, fa.pitch(), s); if (rc_mp) return rc_mp; }
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// the closing average of a head: [N][Cb][H][W][8] -> the C8 matrix [Cb][Mp][8] the cls / bbox GEMM reads
static PoolKernel pick_global_avg(const ResNetGraph *g, const ActI &cur) {
  if (g->bf16 && (g_bf16_fast_pool & 2) && (size_t)16 * cur.H * cur.W * 9 * sizeof(float) <= 64 * 1024) return PK_GAVG_BF16_LDS;
  return g->bf16 ? PK_GAVG_BF16 : PK_GAVG_F32;
}
int rn_global_avg(const ResNetGraph *g, const ActI &cur, int N, float *d_feat_c8, int Mp, hipStream_t s) {
  const size_t total = (size_t)N * cur.Cb() * 2;
  const PoolKernel form = pick_global_avg(g, cur);
  RN_POOL(form);
  switch (form) {
  case PK_GAVG_BF16_LDS:
    hipLaunchKernelGGL(avgpool_c8i_bf16_to_c8_lds_kernel, dim3((unsigned)((N + 15) / 16), (unsigned)cur.Cb()), dim3(256), (size_t)16 * cur.H * cur.W * 9 * sizeof(float), s,
                       reinterpret_cast<const bf16_t *>(cur.p), N, cur.H * cur.W, cur.pitch(), 1.0f / (float)(cur.H * cur.W), d_feat_c8, Mp);
    break;
  case PK_GAVG_BF16:
    hipLaunchKernelGGL(avgpool_c8i_bf16_to_c8_kernel, dim3((unsigned)cdiv_sz(total, 256)), dim3(256), 0, s, reinterpret_cast<const bf16_t *>(cur.p), N, cur.Cb(),
                       cur.H * cur.W, cur.pitch(), 1.0f / (float)(cur.H * cur.W), d_feat_c8, Mp);
    break;
  default:  // PK_GAVG_F32
    hipLaunchKernelGGL(avgpool_c8i_to_c8_kernel, dim3((unsigned)cdiv_sz(total, 256)), dim3(256), 0, s, cur.p, N, cur.Cb(), cur.H * cur.W, cur.pitch(),
                       1.0f / (float)(cur.H * cur.W), d_feat_c8, Mp);
  }
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

// The per-image preparation of the bf16 ROI pooling — the order-preserving int16 image of the feature map and, where a head fuses the
// max-pool of its pooled input, its vertical range-max levels — for head `head` (-1: whatever ANY head needs).  Built once per trunk run
// (the valid flags), on `s`.
int heads_prepare_impl(ResNetGraph *g, int head, hipStream_t s) {
  const int Cb = (g->feat_c + 7) / 8;
  if (!(g->bf16 && fast_pool_ok(g))) return MPN_OK;
  const bool fuse_mp = roi_maxpool_fused(g);
  const ActI fa{g->feat, 1, g->feat_c, g->feat_h, g->feat_w};
  const size_t need = (size_t)Cb * fa.pitch() * 8;
  if (g->feat_sorted_elems < need) {  // first use (or a larger image than any before): outside the steady state
    float *q = reinterpret_cast<float *>(g->feat_sorted);
    g->feat_sorted = nullptr; g->feat_sorted_elems = 0;
    int rc = rn_regrow(g, &q, need * sizeof(bf16_t));
    if (rc) return rc;
    g->feat_sorted = reinterpret_cast<bf16_t *>(q); g->feat_sorted_elems = need; g->feat_sorted_valid = false;
  }
  bool any_mp = false;
  if (fuse_mp)
    for (int h = 0; h < (int)g->g_heads.size(); ++h)
      if (head < 0 || h == head)
        for (const GOp &op : g->g_heads[h]) any_mp = any_mp || op.from_rois;
  const int want_levels = (any_mp && (g_graph_fuse & 64) && g->feat_h > 1) ? 31 - __builtin_clz((unsigned)g->feat_h) : 0;
  if (want_levels > 0 && (g->feat_vmax_elems < need || g->feat_vmax_levels < want_levels)) {  // outside the steady state, as above
    float *q = reinterpret_cast<float *>(g->feat_vmax);
    g->feat_vmax = nullptr; g->feat_vmax_elems = 0; g->feat_vmax_levels = 0;
    int rc = rn_regrow(g, &q, need * sizeof(bf16_t) * want_levels);
    if (rc) return rc;
    g->feat_vmax = reinterpret_cast<bf16_t *>(q); g->feat_vmax_elems = need; g->feat_vmax_levels = want_levels; g->feat_vmax_valid = false;
  }
  if (!g->feat_sorted_valid) {
    hipLaunchKernelGGL(bf16_sortable_kernel, dim3((unsigned)cdiv_sz(need / 8, 256)), dim3(256), 0, s, reinterpret_cast<const u32x4 *>(g->feat), need / 8,
                       reinterpret_cast<u32x4 *>(g->feat_sorted));
    MPN_CHECK_LAUNCH();
    g->feat_sorted_valid = true;
    g->feat_vmax_valid = false;
  }
  if (want_levels > 0 && !g->feat_vmax_valid) {  // once per image: level l from level l - 1 (level 0 = the sortable map)
    for (int l = 1; l <= want_levels; ++l) {
      const u32x4 *prev = l == 1 ? reinterpret_cast<const u32x4 *>(g->feat_sorted)
                                 : reinterpret_cast<const u32x4 *>(g->feat_vmax) + (size_t)(l - 2) * (g->feat_vmax_elems / 8);
      hipLaunchKernelGGL(vmax_level_sorted_kernel, dim3((unsigned)cdiv_sz((size_t)g->feat_h * g->feat_w * Cb, 256)), dim3(256), 0, s, prev,
                         reinterpret_cast<u32x4 *>(g->feat_vmax) + (size_t)(l - 1) * (g->feat_vmax_elems / 8), g->feat_h, g->feat_w, fa.pitch(), Cb, 1 << (l - 1));
      MPN_CHECK_LAUNCH();
    }
    g->feat_vmax_valid = true;
  }
  return MPN_OK;
}

}  // namespace mpn

#ifdef MPN_DEBUG_HOOKS
extern "C" void mpn_debug_set_pool_exp(int v) { mpn::g_pool_exp = v; }
extern "C" void mpn_debug_set_bf16_fast_pool(int v) { mpn::g_bf16_fast_pool = v; }
#endif

#ifdef MPN_DEBUG_HOOKS
// tests/test_gpu_layout_kernels.py: c8i_to_pixel_major_kernel alone, with rn_roi_pool's grid.  Rules: layout_debug.h.
#include "layout_debug.h"
// one C x H x W map in C8I [ceil(C / 8)][pitch][8] -> [H * W][ceil(C / 8) * 8]
extern "C" int mpn_debug_c8i_to_pixel_major(const float *d_c8i, size_t c8i_bytes, int C, int H, int W, float *d_pm, size_t pm_bytes) {
  using namespace mpn;
  MPN_CHECK_ARG(C > 0 && H > 0 && W > 0);
  const ActI fa{const_cast<float *>(d_c8i), 1, C, H, W};
  const int Cb = fa.Cb();
  LDBG_BUF(d_c8i, c8i_bytes, (size_t)Cb * fa.pitch() * 8 * sizeof(float), 16);
  LDBG_BUF(d_pm, pm_bytes, (size_t)H * W * Cb * 8 * sizeof(float), 16);
  hipLaunchKernelGGL(c8i_to_pixel_major_kernel, dim3((unsigned)cdiv_sz((size_t)H * W * Cb * 2, 256)), dim3(256), 0, nullptr, d_c8i, Cb, (size_t)H * W, fa.pitch(),
                     d_pm);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}
#endif
