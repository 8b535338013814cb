// train.hip — training the Fast R-CNN head on the device with the trunk frozen (train.lua:154-158, BBoxRegressionCriterion.lua,
// BatchProviderROI.lua:125-131, engines/Optim.lua).  gfx950 only.
//
// What is built is the reference's opt.train_remove_dropouts = true configuration: no dropout, so a step is deterministic.
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

#include "dense.h"

namespace mpn {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------------------------
// Loss + gradient w.r.t. the head's output
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void train_loss_kernel(const float *__restrict__ head, int B, int C, const float *__restrict__ rois,
                                                         const float *__restrict__ gt, const int *__restrict__ labels, LossCfg cfg,
                                                         float *__restrict__ g, int Mp, float *__restrict__ loss) {
  __shared__ float s_cls[256], s_box[256];
  const int ld = 5 * C, nchunk = (5 * C + 7) / 8;
  const float invB = 1.0f / (float)B, gbox = cfg.bbox_weight / (float)B;
  float acc_cls = 0.0f, acc_box = 0.0f;
  for (int i = threadIdx.x; i < B; i += 256) {  // one row per thread, rows ascending
    const float *z = head + (size_t)i * ld;
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
        d[j] = z[C + 4 * y + j] - tg[j];
        const float a = fabsf(d[j]);
        row += a < 1.0f ? 0.5f * d[j] * d[j] : a - 0.5f;
      }
      acc_box += row;
    }
    const float inv_sum = 1.0f / sum;
    for (int q = 0; q < nchunk; ++q) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int n = q * 8 + e;
        float t = 0.0f;
        if (n < C) t = (expf(z[n] - mx) * inv_sum - (n == y ? 1.0f : 0.0f)) * invB;
        else if (y > 0 && n >= C + 4 * y && n < C + 4 * y + 4) {
          const int j = n - C - 4 * y;
          const float dd = j == 0 ? d[0] : (j == 1 ? d[1] : (j == 2 ? d[2] : d[3]));
          t = gbox * (dd < -1.0f ? -1.0f : (dd > 1.0f ? 1.0f : dd));
        }
        v[e] = t;
      }
      float *o = g + ((size_t)q * Mp + i) * 8;
      *reinterpret_cast<f32x4 *>(o) = f32x4{v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4 *>(o + 4) = f32x4{v[4], v[5], v[6], v[7]};
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

int train_loss(const float *d_head, int B, int C, const float *d_rois, const float *d_gt, const int *d_labels, const LossCfg &cfg,
               float *d_g_c8, int Mp, float *d_loss, hipStream_t s) {
  MPN_CHECK_ARG(d_head && d_rois && d_gt && d_labels && d_g_c8 && d_loss && B > 0 && C > 1 && Mp >= B);
  hipLaunchKernelGGL(train_loss_kernel, dim3(1), dim3(256), 0, s, d_head, B, C, d_rois, d_gt, d_labels, cfg, d_g_c8, Mp, d_loss);
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
// Input gradient: dx = (g W) .* [act > 0]
// ---------------------------------------------------------------------------------------------------------------------------------
struct DgradArgs {
  const float *g, *w, *act;
  float *dx;
  int g_Mp, x_Mp, B, N, NP, nchunks, n_per_wave;
};
constexpr int kDgradLds = 3 * 128 * 64 * 4;  // the partial sums of waves 1..3

// Block = 32 k-chunks (256 k) x 32 rows m; its 4 waves split the contraction over n into four contiguous ranges (n ascending in pairs
// inside a range) and wave 0 adds the four partial sums in wave order: ((s0 + s1) + s2) + s3, the same in every run.  A = packed-weight
// records (i = chunk; the record of (chunk, n) holds W[n][chunk * 8 .. + 8]), B = g[m][n] (j = m).  A lane of wave 0 ends with whole
// records of dx — chunk ck0 + 8 (r / 4) + 4 (lane / 32) + r % 4, row m0 + lane % 32 —, masks them with the forward activation and stores.
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
    const f32x4 a0 = *reinterpret_cast<const f32x4 *>(a.act + off), a1 = *reinterpret_cast<const f32x4 *>(a.act + off + 4);
    f32x4 d0, d1;
#pragma unroll
    for (int e = 0; e < 4; ++e) { d0[e] = a0[e] > 0.0f ? acc[e][r] : 0.0f; d1[e] = a1[e] > 0.0f ? acc[4 + e][r] : 0.0f; }
    *reinterpret_cast<f32x4 *>(a.dx + off) = d0; *reinterpret_cast<f32x4 *>(a.dx + off + 4) = d1;
  }
}

int linear_dgrad_c8(const float *d_g_c8, int g_Mp, int B, int N, const float *d_wpk, int K, const float *d_act_c8, float *d_dx_c8, int x_Mp,
                    hipStream_t s) {
  MPN_CHECK_ARG(d_g_c8 && d_wpk && d_act_c8 && d_dx_c8 && B > 0 && N > 0 && K > 0 && g_Mp >= B && x_Mp >= B);
  DgradArgs a{};
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
  if (!d_w && !d_b) return MPN_OK;
  const size_t total = d_w ? (size_t)(n1 - n0) * K : (size_t)(n1 - n0);
  hipLaunchKernelGGL(unpack_lin_w_kernel, dim3((unsigned)cdiv_sz(total, 256)), dim3(256), 0, s, d_wpk, d_bpk, K, lin_np(N), inner, n0, n1, d_w, d_b);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

}  // namespace mpn
