// layout_debug.hip — the state-free mpn_debug_* pass-throughs to the layout converters, weight packers, image transforms, the halo
// re-layer and the plain 2x2 pool whose launchers a header declares (dense.h, graph_internal.h, pipeline.h); debug flavour only,
// DESIGN.md section 13.17, tests/test_gpu_layout_kernels.py.  The entries of the kernels that are local to a translation unit sit in
// that file (pipeline.hip, graph_pool.hip, resnet.hip).  Rules: layout_debug.h.  Every entry calls the product's own launcher on the
// null stream; maps are laid out as make_act lays a C x H x W map out.
#include "dense.h"
#include "graph_internal.h"
#include "layout_debug.h"
#include "pipeline.h"

#ifdef MPN_DEBUG_HOOKS
using namespace mpn;

static size_t ldbg_c8(int cols, int Mp) { return (size_t)cdiv(cols, 8) * Mp * 8 * sizeof(float); }

extern "C" int mpn_debug_nchw_to_c8p(const float *d_in, size_t in_bytes, int C, int H, int W, float *d_out, size_t out_bytes) {
  MPN_CHECK_ARG(C > 0 && H > 0 && W > 0);
  LDBG_BUF(d_in, in_bytes, (size_t)C * H * W * sizeof(float), 4);
  LDBG_BUF(d_out, out_bytes, act_bytes(C, H, W), 16);
  return nchw_to_c8p(d_in, C, H, W, make_act(d_out, C, H, W), nullptr);
}

extern "C" int mpn_debug_c8p_to_nchw(const float *d_in, size_t in_bytes, int C, int H, int W, float *d_out, size_t out_bytes) {
  MPN_CHECK_ARG(C > 0 && H > 0 && W > 0);
  LDBG_BUF(d_in, in_bytes, act_bytes(C, H, W), 4);
  LDBG_BUF(d_out, out_bytes, (size_t)C * H * W * sizeof(float), 4);
  return c8p_to_nchw(make_act(const_cast<float *>(d_in), C, H, W), d_out, nullptr);
}

// d_c8: [ceil(K / 8)][lin_mp(M)][8]
extern "C" int mpn_debug_rowmajor_to_c8(const float *d_x, size_t x_bytes, int M, int K, float *d_c8, size_t c8_bytes) {
  MPN_CHECK_ARG(M > 0 && K > 0);
  LDBG_BUF(d_x, x_bytes, (size_t)M * K * sizeof(float), 4);
  LDBG_BUF(d_c8, c8_bytes, ldbg_c8(K, lin_mp(M)), 16);
  return rowmajor_to_c8(d_x, M, K, d_c8, nullptr);
}

extern "C" int mpn_debug_c8_to_rowmajor(const float *d_c8, size_t c8_bytes, int M, int N, float *d_y, size_t y_bytes) {
  MPN_CHECK_ARG(M > 0 && N > 0);
  LDBG_BUF(d_c8, c8_bytes, ldbg_c8(N, lin_mp(M)), 4);
  LDBG_BUF(d_y, y_bytes, (size_t)M * N * sizeof(float), 4);
  return c8_to_rowmajor(d_c8, M, N, d_y, nullptr);
}

// pooled C8 matrix [ceil(C / 8) * PP][Mp][8] -> [N, C * PP].  The launcher checks nothing: the shape is checked here.
extern "C" int mpn_debug_unpack_pooled(const float *d_xc8, size_t x_bytes, int N, int C, int PP, int Mp, float *d_out, size_t out_bytes) {
  MPN_CHECK_ARG(N > 0 && C > 0 && PP > 0 && Mp >= N);
  LDBG_BUF(d_xc8, x_bytes, (size_t)cdiv(C, 8) * PP * Mp * 8 * sizeof(float), 4);
  LDBG_BUF(d_out, out_bytes, (size_t)N * C * PP * sizeof(float), 4);
  return launch_unpack_pooled(d_xc8, N, C, PP, Mp, d_out);
}

// d_w [Cout, Cin, 3, 3], d_b [Cout] or null -> d_wpk [ceil(Cin / 8)][9][CoutP][8], d_bpk [CoutP]
extern "C" int mpn_debug_pack_conv_weights(const float *d_w, size_t w_bytes, const float *d_b, size_t b_bytes, int Cin, int Cout, float *d_wpk,
                                           size_t wpk_bytes, float *d_bpk, size_t bpk_bytes) {
  MPN_CHECK_ARG(Cin > 0 && Cout > 0);
  LDBG_BUF(d_w, w_bytes, (size_t)Cout * Cin * 9 * sizeof(float), 4);
  if (d_b) LDBG_BUF(d_b, b_bytes, (size_t)Cout * sizeof(float), 4);
  LDBG_BUF(d_wpk, wpk_bytes, conv_wpk_elems(Cin, Cout) * sizeof(float), 4);
  LDBG_BUF(d_bpk, bpk_bytes, (size_t)conv_coutp(Cout) * sizeof(float), 4);
  return pack_conv_weights(d_w, d_b, Cin, Cout, d_wpk, d_bpk, nullptr);
}

// d_w [Cout, Cin <= 4, 3, 3] -> d_w36 [36][CoutP]
extern "C" int mpn_debug_pack_conv_weights_first(const float *d_w, size_t w_bytes, int Cin, int Cout, float *d_w36, size_t w36_bytes) {
  MPN_CHECK_ARG(Cin > 0 && Cin <= 4 && Cout > 0);
  LDBG_BUF(d_w, w_bytes, (size_t)Cout * Cin * 9 * sizeof(float), 4);
  LDBG_BUF(d_w36, w36_bytes, conv_first_elems(Cout) * sizeof(float), 4);
  return pack_conv_weights_first(d_w, Cin, Cout, d_w36, nullptr);
}

// The launchers take `swap` as given: a plane index outside 0..2 would read outside the image, so it is refused here.
static bool ldbg_swap_ok(const int *swap) {
  if (!swap) return false;
  for (int j = 0; j < 3; ++j) if (swap[j] < 0 || swap[j] > 2) return false;
  return true;
}

// d_in [3, H, W] -> the one-block C8P map of an Hc x Wc canvas.  canvas = 0: image_transform_c8p (Hc == H and Wc == W are its own
// check); 1: image_transform_canvas_c8p.
extern "C" int mpn_debug_image_transform_c8p(const float *d_in, size_t in_bytes, int H, int W, const int *swap, double scale, const double *mean,
                                             const double *std, int has_std, int canvas, int Hc, int Wc, float *d_out, size_t out_bytes) {
  MPN_CHECK_ARG(H > 0 && W > 0 && Hc > 0 && Wc > 0 && mean && std && (canvas == 0 || canvas == 1));
  MPN_CHECK_ARG(ldbg_swap_ok(swap));
  LDBG_BUF(d_in, in_bytes, (size_t)3 * H * W * sizeof(float), 4);
  LDBG_BUF(d_out, out_bytes, act_bytes(3, Hc, Wc), 16);
  const Act out = make_act(d_out, 3, Hc, Wc);
  return canvas ? image_transform_canvas_c8p(d_in, H, W, swap, scale, mean, std, has_std, out, nullptr)
                : image_transform_c8p(d_in, H, W, swap, scale, mean, std, has_std, out, nullptr);
}

// n maps, map i the C[i] x H[i] x W[i] map at ptrs[i] (host arrays).  n = 0 launches nothing.
extern "C" int mpn_debug_c8p_zero_halos(int n, float *const *ptrs, const size_t *bytes, const int *C, const int *H, const int *W) {
  MPN_CHECK_ARG(n >= 0 && n <= 4096 && (n == 0 || (ptrs && bytes && C && H && W)));
  std::vector<Act> acts((size_t)n + 1);  // (+ 1: c8p_zero_halos wants a table even for n = 0)
  for (int i = 0; i < n; ++i) {
    MPN_CHECK_ARG(C[i] > 0 && H[i] > 0 && W[i] > 0);
    float *d_map = ptrs[i];
    LDBG_BUF(d_map, bytes[i], act_bytes(C[i], H[i], W[i]), 16);
    acts[i] = make_act(d_map, C[i], H[i], W[i]);
  }
  return c8p_zero_halos(acts.data(), n, nullptr);
}

// d_in [C, H, W] and d_out [C, ceil(H / 2), ceil(W / 2)] as make_act lays them out
extern "C" int mpn_debug_maxpool2x2_c8p(const float *d_in, size_t in_bytes, int C, int H, int W, float *d_out, size_t out_bytes) {
  MPN_CHECK_ARG(C > 0 && H > 0 && W > 0);
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  LDBG_BUF(d_in, in_bytes, act_bytes(C, H, W), 16);
  LDBG_BUF(d_out, out_bytes, act_bytes(C, Ho, Wo), 16);
  return maxpool2x2_c8p(make_act(const_cast<float *>(d_in), C, H, W), make_act(d_out, C, Ho, Wo), nullptr);
}

// ---- the graph executor's side (graph_internal.h) ---------------------------------------------------------------------------------------
static size_t ldbg_c8i(int C, int H, int W) { return (size_t)cdiv(C, 8) * (ActI{nullptr, 1, C, H, W}).pitch() * 8 * sizeof(float); }

// one C x H x W map: its C8I form [ceil(C / 8)][pitch = H * W rounded up to 128][8] and its C8P form.  to_c8p = 1: rn_c8i_to_c8p, 0: back.
extern "C" int mpn_debug_c8i_c8p(float *d_c8i, size_t c8i_bytes, float *d_c8p, size_t c8p_bytes, int C, int H, int W, int to_c8p) {
  MPN_CHECK_ARG(C > 0 && H > 0 && W > 0 && (to_c8p == 0 || to_c8p == 1));
  LDBG_BUF(d_c8i, c8i_bytes, ldbg_c8i(C, H, W), 16);
  LDBG_BUF(d_c8p, c8p_bytes, act_bytes(C, H, W), 16);
  GTensor t;
  t.C = C; t.H = H; t.W = W; t.buf = d_c8i; t.c8p = d_c8p;
  return to_c8p ? rn_c8i_to_c8p(t, nullptr) : rn_c8p_to_c8i(t, nullptr);
}

// rn_image_transform on a graph that holds nothing but the two image buffers.  fp32: d_img [H * W][8] floats, d_planar [3][H][W] or null.
// bf16: d_img two planes [2][pitch][8] of 16-bit values, d_planar not used.
extern "C" int mpn_debug_image_transform_c8i(const float *d_in, size_t in_bytes, int H, int W, const int *swap, double scale, const double *mean,
                                             const double *std, int has_std, int bf16, void *d_img, size_t img_bytes, float *d_planar,
                                             size_t planar_bytes) {
  MPN_CHECK_ARG(H > 0 && W > 0 && mean && std && (bf16 == 0 || bf16 == 1));
  MPN_CHECK_ARG(ldbg_swap_ok(swap));
  LDBG_BUF(d_in, in_bytes, (size_t)3 * H * W * sizeof(float), 4);
  const size_t pitch = (ActI{nullptr, 1, 3, H, W}).pitch();
  LDBG_BUF(d_img, img_bytes, bf16 ? 2 * pitch * 8 * sizeof(bf16_t) : (size_t)H * W * 8 * sizeof(float), 16);
  if (d_planar && !bf16) LDBG_BUF(d_planar, planar_bytes, (size_t)3 * H * W * sizeof(float), 4);
  ResNetGraph g;
  g.bf16 = bf16 != 0;
  g.img = static_cast<float *>(d_img);
  g.img_planar = bf16 ? nullptr : d_planar;
  return rn_image_transform(&g, d_in, H, W, swap, scale, mean, std, has_std, nullptr);
}

#endif
