// resnet_debug.hip — the graph executor's test and timing entry points (mpn_debug_*): compiled to nothing without MPN_DEBUG_HOOKS.
// The setter of a knob that one file alone reads sits beside the knob, in that file; the shared knobs' setters are here.
#include "graph_internal.h"

#ifdef MPN_DEBUG_HOOKS
// Kernel-only timing of ONE per-ROI bf16 convolution (rn_conv, per_roi dispatch) on a batch of B maps of H x W (tools/bench_conv_bf16.py):
// random bf16 activations / weights (zero operands clock higher), optional residual; returns the average ms of `iters` launches.
namespace mpn {
__global__ void checksum_u16_kernel(const unsigned short *__restrict__ p, size_t n, unsigned long long *__restrict__ acc) {
  unsigned long long local = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    local += (unsigned long long)p[i] * (unsigned long long)(i % 65521u + 1u);
  atomicAdd(acc, local);
}
}  // namespace mpn
// checksum_out (optional): a position-weighted 64-bit checksum of the (zero-initialised, then written) output tensor — equal checksums
// under two kernel choices = the same bits
extern "C" int mpn_debug_bench_conv_bf16(int Cin, int Cout, int KH, int KW, int sh, int sw, int ph, int pw, int B, int H, int W, int with_res, int iters,
                                         float *ms_out, unsigned long long *checksum_out) {
  using namespace mpn;
  MPN_CHECK_ARG(Cin > 0 && Cout > 0 && KH > 0 && KW > 0 && B > 0 && H > 0 && W > 0 && iters > 0 && ms_out);
  ResNetGraph *g = new ResNetGraph();
  g->bf16 = true;
  RnConv c;
  c.Cin = Cin; c.Cout = Cout; c.KH = KH; c.KW = KW; c.sh = sh; c.sw = sw; c.ph = ph; c.pw = pw; c.K = KH; c.stride = sh; c.pad = ph;
  const size_t nw = (size_t)Cout * Cin * KH * KW;
  std::vector<float> hw(nw);
  unsigned x = 2463534242u;
  for (auto &v : hw) { x = x * 1664525u + 1013904223u; v = ((x >> 8) * (1.0f / 8388608.0f) - 1.0f) * 0.05f; }
  float *d_w = nullptr;
  int rc = rn_alloc(g, &d_w, nw * sizeof(float));
  if (rc == MPN_OK && hipMemcpy(d_w, hw.data(), nw * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) rc = MPN_EHIP;
  if (rc == MPN_OK) rc = rn_pack(g, c, d_w, nullptr);
  const int OH = (H + 2 * ph - KH) / sh + 1, OW = (W + 2 * pw - KW) / sw + 1;
  const size_t ie = c8i_elems(B, Cin, H, W), oe = c8i_elems(B, Cout, OH, OW);
  float *in = nullptr, *out = nullptr, *res = nullptr;
  if (rc == MPN_OK) rc = rn_alloc(g, &in, ie * sizeof(bf16_t));
  if (rc == MPN_OK) rc = rn_alloc(g, &out, oe * sizeof(bf16_t));
  if (rc == MPN_OK && with_res) rc = rn_alloc(g, &res, oe * sizeof(bf16_t));
  if (rc == MPN_OK) {
    std::vector<unsigned short> hi(std::max(ie, oe));
    for (auto &v : hi) { x = x * 1664525u + 1013904223u; v = (unsigned short)(0x3c00u + ((x >> 9) & 0x3ffu) + ((x >> 31) << 15)); }  // +-[0.0078, 0.031): finite bf16
    { const char *fill = getenv("MPN_BENCH_FILL"); if (fill && fill[0] == 'z') for (auto &v : hi) v = 0; }  // DVFS experiments: zero activations clock higher
    if (hipMemcpy(in, hi.data(), ie * sizeof(bf16_t), hipMemcpyHostToDevice) != hipSuccess) rc = MPN_EHIP;
    if (rc == MPN_OK && res && hipMemcpy(res, hi.data(), oe * sizeof(bf16_t), hipMemcpyHostToDevice) != hipSuccess) rc = MPN_EHIP;
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (rc == MPN_OK && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) rc = MPN_EHIP;
  const ActI ai{in, B, Cin, H, W};
  ActI o;
  for (int i = 0; i < 2 && rc == MPN_OK; ++i) rc = rn_conv(c, ai, out, res, 1, nullptr, &o, true, true);
  if (rc == MPN_OK && hipDeviceSynchronize() != hipSuccess) rc = MPN_EHIP;
  if (rc == MPN_OK && checksum_out) {
    unsigned long long *d_acc = nullptr;
    if (hipMalloc(&d_acc, 8) != hipSuccess || hipMemset(d_acc, 0, 8) != hipSuccess || hipMemset(out, 0, oe * sizeof(bf16_t)) != hipSuccess) rc = MPN_EHIP;
    if (rc == MPN_OK) rc = rn_conv(c, ai, out, res, 1, nullptr, &o, true, true);
    if (rc == MPN_OK) {
      hipLaunchKernelGGL(checksum_u16_kernel, dim3(2048), dim3(256), 0, nullptr, reinterpret_cast<const unsigned short *>(out), oe, d_acc);
      if (hipMemcpy(checksum_out, d_acc, 8, hipMemcpyDeviceToHost) != hipSuccess) rc = MPN_EHIP;
    }
    if (d_acc) (void)hipFree(d_acc);
  }
  if (rc == MPN_OK) (void)hipEventRecord(e0, nullptr);
  for (int i = 0; i < iters && rc == MPN_OK; ++i) rc = rn_conv(c, ai, out, res, 1, nullptr, &o, true, true);
  if (rc == MPN_OK) {
    (void)hipEventRecord(e1, nullptr);
    float ms = 0.f;
    if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = MPN_EHIP;
    *ms_out = ms / iters;
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  resnet_free(g);
  return rc;
}
// Test hook (tests/test_gpu_conv_numerics.py): ONE convolution through rn_conv, on NCHW fp32 device operands x [B, Cin, H, W], w [Cout, Cin,
// KH, KW], b [Cout] (optional), res [B, Cout, OH, OW] (optional), packed by rn_pack into a scratch graph as graph building packs them
// (lin_w / col_w; with `mosaic`, fp32 3x3 / stride-1 / pad-1 layers also get the Winograd weights and mosaic images for max_rois maps, as
// mpn_resnet_create sets them up).  bf16: x, res and the weights round to bf16 (RNE), as the graph stores them.  The C8I input's pad channel
// planes and its rows from B*H*W up to the pitch hold the finite pattern pad_fill * (+-1 .. 5); so do the residual's.  The output goes to
// channels [out_c_off, out_c_off + Cout) of an out_c-channel C8I tensor (out_c_off: a multiple of 8) whose every element first holds the
// sentinel NaN 0x7fa5a5a5 (bf16: 0x7fa5).  The rn_conv call is repeated for the batch sizes n_b[0 .. n_rep - 1] (each the first maps of x;
// a fresh layout per run, one graph: the mosaic images carry over); y [n_b[n_rep - 1], Cout, OH, OW] fp32 is the last run's output.  raw
// (optional, raw_cap bytes): the last run's whole output buffer, raw_bytes (optional) its size.  form_out: mpn_debug_conv_last_form().
namespace mpn {
__global__ void dbg_nchw_to_c8i_kernel(const float *__restrict__ x, int B, int C, int H, int W, size_t pitch, size_t total, float pad_fill, int bf16,
                                       void *__restrict__ out, int one_sign = 0) {  // one_sign: the pad pattern is pad_fill * (1 .. 5)
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int j = (int)(t & 7);
  const size_t r = (t >> 3) % pitch;
  const int c = (int)((t >> 3) / pitch) * 8 + j;
  const size_t HW = (size_t)H * W;
  float v = pad_fill * (float)(1 + (int)(t % 5)) * ((t & 8) && !one_sign ? -1.0f : 1.0f);
  if (c < C && r < (size_t)B * HW) v = x[((r / HW) * C + c) * HW + r % HW];
  if (bf16) static_cast<bf16_t *>(out)[t] = f2bf(v);
  else static_cast<float *>(out)[t] = v;
}
__global__ void dbg_c8i_to_nchw_kernel(const void *__restrict__ in, int B, int C, int H, int W, size_t pitch, int cb0, int bf16, float *__restrict__ y) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t HW = (size_t)H * W;
  if (t >= (size_t)B * C * HW) return;
  const size_t b = t / ((size_t)C * HW), rem = t % ((size_t)C * HW);
  const int c = (int)(rem / HW);
  const size_t off = ((size_t)(cb0 + c / 8) * pitch + b * HW + rem % HW) * 8 + c % 8;
  y[t] = bf16 ? bf2f(static_cast<const bf16_t *>(in)[off]) : static_cast<const float *>(in)[off];
}
__global__ void dbg_fill_u32_kernel(unsigned *p, size_t n, unsigned v) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) p[t] = v;
}
}  // namespace mpn
extern "C" int mpn_debug_conv_last_form(void) { return mpn::g_dbg_conv_form; }
extern "C" int mpn_debug_conv_form(const float *d_x, int Cin, int H, int W, const float *d_w, int Cout, int KH, int KW, int sh, int sw, int ph, int pw,
                                   const float *d_b, const float *d_res, int relu, int norelu_c0, int norelu_c1, int bf16, int per_roi, int allow_gemm,
                                   int mosaic, int max_rois, int n_rep, const int *n_b, int out_c, int out_c_off, float pad_fill, float *d_y, void *d_raw,
                                   size_t raw_cap, size_t *raw_bytes, int *form_out) {
  using namespace mpn;
  MPN_CHECK_ARG(d_x && d_w && d_y && Cin > 0 && H > 0 && W > 0 && Cout > 0 && KH > 0 && KW > 0 && sh > 0 && sw > 0 && ph >= 0 && pw >= 0);
  MPN_CHECK_ARG(n_rep >= 1 && n_b && out_c_off >= 0 && out_c_off % 8 == 0 && out_c >= out_c_off + Cout && norelu_c0 % 8 == 0 && norelu_c1 % 8 == 0);
  for (int i = 0; i < n_rep; ++i) MPN_CHECK_ARG(n_b[i] > 0);
  const int OH = (H + 2 * ph - KH) / sh + 1, OW = (W + 2 * pw - KW) / sw + 1;
  MPN_CHECK_ARG(OH > 0 && OW > 0 && std::isfinite(pad_fill));
  MPN_CHECK_HIP(hipDeviceSynchronize());
  ResNetGraph *g = new ResNetGraph();
  g->bf16 = bf16 != 0;
  const size_t esz = g->bf16 ? sizeof(bf16_t) : sizeof(float);
  RnConv c;
  c.Cin = Cin; c.Cout = Cout; c.KH = KH; c.KW = KW; c.sh = sh; c.sw = sw; c.ph = ph; c.pw = pw; c.K = KH; c.stride = sh; c.pad = ph;
  c.norelu_c0 = norelu_c0; c.norelu_c1 = norelu_c1;
  int rc = rn_pack(g, c, d_w, d_b);
  if (rc == MPN_OK && mosaic && !g->bf16 && (g_graph_fuse & 128) && KH == 3 && KW == 3 && sh == 1 && sw == 1 && ph == 1 && pw == 1 && Cin % 8 == 0 &&
      Cout % 8 == 0 && Cin >= 16 && max_rois > 0) {  // as mpn_resnet_create: the Winograd weights and the two zeroed mosaic images
    rc = rn_alloc(g, &c.wino, conv_wino_elems(Cin, Cout) * sizeof(float));
    if (rc == MPN_OK) rc = pack_conv_weights_wino(d_w, Cin, Cout, c.wino, nullptr);
    const int mx = std::max(1, 32 / (W + 1)), rows = ((max_rois + mx - 1) / mx) * (H + 1), cols = mx * (W + 1);
    if (rc == MPN_OK) rc = rn_alloc(g, &c.mos_in, act_bytes(Cin, rows, cols));
    if (rc == MPN_OK) rc = rn_alloc(g, &c.mos_out, act_bytes(Cout, rows, cols));
    if (rc == MPN_OK && (hipMemset(c.mos_in, 0, act_bytes(Cin, rows, cols)) != hipSuccess || hipMemset(c.mos_out, 0, act_bytes(Cout, rows, cols)) != hipSuccess))
      rc = MPN_EHIP;
    c.mos_h = H; c.mos_w = W; c.mos_mx = mx; c.mos_rows = rows; c.mos_cols = cols;
  }
  // the output's channel blocks: the wider tensor's, and room for a form that writes whole 128-channel panels from out_c_off on
  const int ob_all = std::max(round_up(out_c, 128), out_c_off + round_up(Cout, 128)) / 8;
  float *in = nullptr, *out = nullptr, *res = nullptr;
  for (int i = 0; i < n_rep && rc == MPN_OK; ++i) {
    const int B = n_b[i];
    if (in) { (void)hipFree(in); in = nullptr; }
    if (out) { (void)hipFree(out); out = nullptr; }
    if (res) { (void)hipFree(res); res = nullptr; }
    const size_t ie = c8i_elems(B, Cin, H, W), pitch_o = ((size_t)B * OH * OW + 127) / 128 * 128, oe = (size_t)ob_all * pitch_o * 8;
    const size_t re = c8i_elems(B, Cout, OH, OW);
    if (hipMalloc(&in, ie * esz) != hipSuccess || hipMalloc(&out, oe * esz) != hipSuccess || (d_res && hipMalloc(&res, re * esz) != hipSuccess)) {
      rc = MPN_EHIP;
      break;
    }
    const ActI ai0{in, B, Cin, H, W};
    hipLaunchKernelGGL(dbg_nchw_to_c8i_kernel, dim3((unsigned)cdiv_sz(ie, 256)), dim3(256), 0, nullptr, d_x, B, Cin, H, W, ai0.pitch(), ie, pad_fill, bf16, in);
    MPN_CHECK_LAUNCH();
    if (res) {
      hipLaunchKernelGGL(dbg_nchw_to_c8i_kernel, dim3((unsigned)cdiv_sz(re, 256)), dim3(256), 0, nullptr, d_res, B, Cout, OH, OW, pitch_o, re, pad_fill, bf16, res);
      MPN_CHECK_LAUNCH();
    }
    if (g->bf16) {
      hipLaunchKernelGGL(dbg_fill_u32_kernel, dim3((unsigned)cdiv_sz(oe / 2, 256)), dim3(256), 0, nullptr, reinterpret_cast<unsigned *>(out), oe / 2, 0x7fa57fa5u);
    } else {
      hipLaunchKernelGGL(dbg_fill_u32_kernel, dim3((unsigned)cdiv_sz(oe, 256)), dim3(256), 0, nullptr, reinterpret_cast<unsigned *>(out), oe, 0x7fa5a5a5u);
    }
    MPN_CHECK_LAUNCH();
    ActI ai{in, B, Cin, H, W};
    if (Cin == 3 && B == 1) ai.planar = d_x;  // the image layer: the graph keeps the same pixels as [3][H][W] planes
    ActI o;
    g_dbg_conv_form = 0;
    rc = rn_conv(c, ai, reinterpret_cast<float *>(reinterpret_cast<char *>(out) + (size_t)(out_c_off / 8) * pitch_o * 8 * esz), res, relu, nullptr, &o,
                 allow_gemm != 0, per_roi != 0);
    if (rc == MPN_OK && hipDeviceSynchronize() != hipSuccess) rc = MPN_EHIP;
    if (rc == MPN_OK && i + 1 == n_rep) {
      const size_t total = (size_t)B * Cout * OH * OW;
      hipLaunchKernelGGL(dbg_c8i_to_nchw_kernel, dim3((unsigned)cdiv_sz(total, 256)), dim3(256), 0, nullptr, out, B, Cout, OH, OW, pitch_o, out_c_off / 8, bf16, d_y);
      MPN_CHECK_LAUNCH();
      if (raw_bytes) *raw_bytes = oe * esz;
      if (d_raw && raw_cap < oe * esz) { set_error("mpn_debug_conv_form: raw needs %zu bytes", oe * esz); rc = MPN_EINVAL; }
      else if (d_raw) MPN_CHECK_HIP(hipMemcpy(d_raw, out, oe * esz, hipMemcpyDeviceToDevice));
    }
  }
  if (form_out) *form_out = g_dbg_conv_form;
  if (rc == MPN_OK && hipDeviceSynchronize() != hipSuccess) rc = MPN_EHIP;
  if (in) (void)hipFree(in);
  if (out) (void)hipFree(out);
  if (res) (void)hipFree(res);
  resnet_free(g);
  return rc;
}

// Test hooks (tests/test_gpu_graph_pool_numerics.py): the pooling, LRN and ROI-pooling launches of the graph executor, one at a time, through
// the dispatch code the product runs (graph_parse / graph_dims / graph_run, resnet_head_forward) on a scratch graph.
//
// mpn_debug_graph_op: ONE op of kind 1 (max-pool), 2 (average pool; op->b = the commuted pool's bias, with op->relu) or 3 (LRN) on the NCHW fp32
// device tensor x [B, C, H, W]; the op reads channels [op->src_c_off, + op->cin) of it (op->src / dst / dst_c_off / w / cout are ignored).  The
// source is laid out as C8I (bf16: rounded RNE) with the finite one-signed pattern pad_fill * (1 .. 5) in the pad lanes of a ragged last channel block,
// in its pad planes and in the rows from B*H*W up to the pitch; the destination is an out_c-channel tensor written at out_c_off whose every
// element first holds the sentinel NaN 0x7fa5a5a5 (bf16: 0x7fa5).  y [B, op->cin, OH, OW] fp32 (y_cap elements), oh / ow the output size,
// raw (optional, raw_cap bytes) the whole output buffer [round_up(out_c, 128) / 8][pitch][8], kernel_out the PoolKernel id that ran.
extern "C" int mpn_debug_graph_op(const float *d_x, int B, int C, int H, int W, const mpn_graph_op *op_in, int bf16, int out_c, int out_c_off, float pad_fill,
                                  float *d_y, size_t y_cap, int *oh_out, int *ow_out, void *d_raw, size_t raw_cap, size_t *raw_bytes, int *kernel_out) {
  using namespace mpn;
  MPN_CHECK_ARG(d_x && d_y && op_in && B > 0 && C > 0 && H > 0 && W > 0 && out_c > 0 && out_c_off >= 0 && std::isfinite(pad_fill));
  MPN_CHECK_ARG(op_in->kind >= 1 && op_in->kind <= 3);
  MPN_CHECK_HIP(hipDeviceSynchronize());
  ResNetGraph *g = new ResNetGraph();
  g->is_graph = true; g->bf16 = bf16 != 0;
  const size_t esz = g->bf16 ? sizeof(bf16_t) : sizeof(float);
  mpn_graph_op o = *op_in;
  o.src = 0; o.dst = 1; o.dst_c_off = out_c_off; o.w = nullptr; o.cout = 0;
  const int tc[2] = {C, out_c};
  std::vector<GOp> ops;
  int rc = graph_parse(g, 1, &o, 2, tc, ops, g->t_head, true);
  if (rc == MPN_OK) rc = graph_dims(ops, g->t_head, H, W);
  size_t oe = 0, pitch_o = 0;
  int OH = 0, OW = 0;
  if (rc == MPN_OK) {
    GTensor &ti = g->t_head[0], &to = g->t_head[1];
    OH = to.H; OW = to.W;
    const ActI ai{nullptr, B, C, H, W}, ao{nullptr, B, out_c, OH, OW};
    const size_t ie = c8i_elems(B, C, H, W);
    pitch_o = ao.pitch(); oe = c8i_elems(B, out_c, OH, OW);
    if ((size_t)B * o.cin * OH * OW > y_cap) { set_error("mpn_debug_graph_op: y needs %zu elements", (size_t)B * o.cin * OH * OW); rc = MPN_EINVAL; }
    if (rc == MPN_OK) rc = rn_alloc(g, &ti.buf, ie * esz);
    if (rc == MPN_OK) rc = rn_alloc(g, &to.buf, oe * esz);
    if (rc == MPN_OK) {
      hipLaunchKernelGGL(dbg_nchw_to_c8i_kernel, dim3((unsigned)cdiv_sz(ie, 256)), dim3(256), 0, nullptr, d_x, B, C, H, W, ai.pitch(), ie, pad_fill, bf16, ti.buf, 1);
      if (g->bf16) hipLaunchKernelGGL(dbg_fill_u32_kernel, dim3((unsigned)cdiv_sz(oe / 2, 256)), dim3(256), 0, nullptr, reinterpret_cast<unsigned *>(to.buf), oe / 2, 0x7fa57fa5u);
      else hipLaunchKernelGGL(dbg_fill_u32_kernel, dim3((unsigned)cdiv_sz(oe, 256)), dim3(256), 0, nullptr, reinterpret_cast<unsigned *>(to.buf), oe, 0x7fa5a5a5u);
      if (hipGetLastError() != hipSuccess) rc = MPN_EHIP;
    }
  }
  g_dbg_pool_kernel[0] = 0;
  if (rc == MPN_OK) rc = graph_run(g, ops, g->t_head, B, nullptr);
  if (rc == MPN_OK && hipDeviceSynchronize() != hipSuccess) rc = MPN_EHIP;
  if (rc == MPN_OK) {
    const size_t total = (size_t)B * o.cin * OH * OW;
    hipLaunchKernelGGL(dbg_c8i_to_nchw_kernel, dim3((unsigned)cdiv_sz(total, 256)), dim3(256), 0, nullptr, g->t_head[1].buf, B, o.cin, OH, OW, pitch_o, out_c_off / 8, bf16, d_y);
    if (hipGetLastError() != hipSuccess) rc = MPN_EHIP;
  }
  if (rc == MPN_OK) {
    if (oh_out) *oh_out = OH;
    if (ow_out) *ow_out = OW;
    if (raw_bytes) *raw_bytes = oe * esz;
    if (kernel_out) *kernel_out = g_dbg_pool_kernel[0];
    if (d_raw && raw_cap < oe * esz) { set_error("mpn_debug_graph_op: raw needs %zu bytes", oe * esz); rc = MPN_EINVAL; }
    else if (d_raw && hipMemcpy(d_raw, g->t_head[1].buf, oe * esz, hipMemcpyDeviceToDevice) != hipSuccess) rc = MPN_EHIP;
  }
  if (hipDeviceSynchronize() != hipSuccess && rc == MPN_OK) rc = MPN_EHIP;
  resnet_free(g);
  return rc;
}
// mpn_debug_head_pool: resnet_head_forward on a scratch graph head without convolutions — the ROI pooling of the one-map NCHW fp32 feature
// [C, H, W] (laid out as above, pad_fill in its pad lanes / planes / rows) for the table d_rois [N][roi_stride] into head tensor 0, optionally ONE
// max-pool op of it (op_in: kind 1 reading all C channels of tensor 0 into tensor 1; from_rois by graph_build's rule, so the fused kernel takes it
// where resnet_head_forward fuses), and the closing average of tensor 0 into the C8 matrix d_c8 [Cb][Mp][8] (pre-filled with the sentinel).
// Every head tensor first holds the sentinel.  d_pooled [N, C, pooled, pooled], d_mp [N, C, OH, OW] (with op_in; mp_cap elements) fp32;
// kernels_out[4] = the PoolKernel ids of {graph_run's op, ROI pooling, fused max-pool, closing average} (0 = none ran), levels_out = the range-max
// levels built.  The fully-connected route (roi_pool_pm) needs an fc_w op and is not reachable from here.
extern "C" int mpn_debug_head_pool(const float *d_feat, int C, int H, int W, const float *d_rois, int roi_stride, int N, int pooled, float spatial_scale,
                                   int roi_bins, int bf16, const mpn_graph_op *op_in, float pad_fill, int Mp, float *d_pooled, float *d_mp, size_t mp_cap,
                                   int *oh_out, int *ow_out, float *d_c8, int *kernels_out, int *levels_out) {
  using namespace mpn;
  MPN_CHECK_ARG(d_feat && d_rois && d_pooled && d_c8 && C > 0 && H > 0 && W > 0 && N > 0 && pooled > 0 && Mp >= N && roi_stride >= 5);
  MPN_CHECK_ARG((roi_bins == MPN_ROI_BINS_CAFFE || roi_bins == MPN_ROI_BINS_ADAPTIVE) && std::isfinite(pad_fill) && (!op_in || (op_in->kind == 1 && d_mp)));
  MPN_CHECK_HIP(hipDeviceSynchronize());
  ResNetGraph *g = new ResNetGraph();
  g->is_graph = true; g->bf16 = bf16 != 0; g->feat_c = C; g->feat_h = H; g->feat_w = W; g->pooled = pooled; g->max_rois = N; g->roi_bins = roi_bins;
  g->out_tensor = 0; g->heads.resize(1); g->g_heads.resize(1);
  const size_t esz = g->bf16 ? sizeof(bf16_t) : sizeof(float);
  const int Cb = (C + 7) / 8;
  int rc = MPN_OK;
  if (op_in) {
    mpn_graph_op o = *op_in;
    o.src = 0; o.dst = 1; o.dst_c_off = 0; o.src_c_off = 0; o.cin = C; o.w = nullptr; o.cout = 0;
    const int tc[2] = {C, C};
    rc = graph_parse(g, 1, &o, 2, tc, g->g_heads[0], g->t_head, true);
    if (rc == MPN_OK)
      for (GOp &op : g->g_heads[0])
        if (MPN_GOP_POOLS_ROIS(op, g->t_head[0].C))
          op.from_rois = true;
  } else {
    g->t_head.resize(1);
    g->t_head[0].C = C;
  }
  if (rc == MPN_OK) rc = graph_dims(g->g_heads[0], g->t_head, pooled, pooled);
  const size_t fe = c8i_elems(1, C, H, W);
  float *feat = nullptr;
  if (rc == MPN_OK) rc = rn_alloc(g, &feat, fe * esz);
  if (rc == MPN_OK) {
    const ActI fa{nullptr, 1, C, H, W};
    hipLaunchKernelGGL(dbg_nchw_to_c8i_kernel, dim3((unsigned)cdiv_sz(fe, 256)), dim3(256), 0, nullptr, d_feat, 1, C, H, W, fa.pitch(), fe, pad_fill, bf16, feat, 1);
    if (hipGetLastError() != hipSuccess) rc = MPN_EHIP;
    g->feat = feat;
  }
  for (size_t i = 0; rc == MPN_OK && i < g->t_head.size(); ++i) {
    GTensor &t = g->t_head[i];
    const size_t te = c8i_elems(N, t.C, t.H, t.W);
    rc = rn_alloc(g, &t.buf, te * esz);
    if (rc != MPN_OK) break;
    hipLaunchKernelGGL(dbg_fill_u32_kernel, dim3((unsigned)cdiv_sz(te * esz / 4, 256)), dim3(256), 0, nullptr, reinterpret_cast<unsigned *>(t.buf), te * esz / 4,
                       g->bf16 ? 0x7fa57fa5u : 0x7fa5a5a5u);
    if (hipGetLastError() != hipSuccess) rc = MPN_EHIP;
  }
  if (rc == MPN_OK) {
    const size_t ce = (size_t)Cb * Mp * 8;
    hipLaunchKernelGGL(dbg_fill_u32_kernel, dim3((unsigned)cdiv_sz(ce, 256)), dim3(256), 0, nullptr, reinterpret_cast<unsigned *>(d_c8), ce, 0x7fa5a5a5u);
    if (hipGetLastError() != hipSuccess) rc = MPN_EHIP;
  }
  if (rc == MPN_OK && g->t_head.size() > 1 && (size_t)N * C * g->t_head[1].H * g->t_head[1].W > mp_cap) {
    set_error("mpn_debug_head_pool: mp needs %zu elements", (size_t)N * C * g->t_head[1].H * g->t_head[1].W);
    rc = MPN_EINVAL;
  }
  for (int i = 0; i < 4; ++i) g_dbg_pool_kernel[i] = 0;
  if (rc == MPN_OK) rc = resnet_head_forward(g, 0, d_rois, roi_stride, N, spatial_scale, d_c8, Mp, nullptr, 0);
  if (rc == MPN_OK && hipDeviceSynchronize() != hipSuccess) rc = MPN_EHIP;
  if (rc == MPN_OK) {
    const ActI pa{nullptr, N, C, pooled, pooled};
    const size_t total = (size_t)N * C * pooled * pooled;
    hipLaunchKernelGGL(dbg_c8i_to_nchw_kernel, dim3((unsigned)cdiv_sz(total, 256)), dim3(256), 0, nullptr, g->t_head[0].buf, N, C, pooled, pooled, pa.pitch(), 0, bf16, d_pooled);
    if (g->t_head.size() > 1) {
      const GTensor &t = g->t_head[1];
      const ActI ma{nullptr, N, C, t.H, t.W};
      const size_t tot2 = (size_t)N * C * t.H * t.W;
      hipLaunchKernelGGL(dbg_c8i_to_nchw_kernel, dim3((unsigned)cdiv_sz(tot2, 256)), dim3(256), 0, nullptr, t.buf, N, C, t.H, t.W, ma.pitch(), 0, bf16, d_mp);
      if (oh_out) *oh_out = t.H;
      if (ow_out) *ow_out = t.W;
    }
    if (hipGetLastError() != hipSuccess) rc = MPN_EHIP;
    if (kernels_out) for (int i = 0; i < 4; ++i) kernels_out[i] = g_dbg_pool_kernel[i];
    if (levels_out) *levels_out = g->feat_vmax_valid ? g->feat_vmax_levels : 0;
  }
  if (hipDeviceSynchronize() != hipSuccess && rc == MPN_OK) rc = MPN_EHIP;
  resnet_free(g);
  return rc;
}
extern "C" void mpn_debug_set_tower_knock(int v) { mpn::g_tower_knock = v; }
extern "C" void mpn_debug_set_roi_invariant(int v) { mpn::g_roi_invariant = v; }
extern "C" void mpn_debug_set_graph_fuse(int v) { mpn::g_graph_fuse = v; }
#endif  // MPN_DEBUG_HOOKS
