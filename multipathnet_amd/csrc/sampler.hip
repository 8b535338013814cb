// sampler.hip — drawing a training minibatch's rows on the device (include/mpn.h mpn_attach_proposals / mpn_sample_rois; DESIGN.md
// section 13.11): DataSetCOCO:attachProposals (DataSetJSON.lua:280-390) with its crowd branch, and BatchProviderROI's setupOne +
// selectBBoxesOne (BatchProviderROI.lua:39-49, 98-101; BatchProviderBase.lua:54-107) for ONE image.  gfx950 only.
//
// Both kernels are latency-class: one launch each, no atomics, no host round trip, every order fixed — the same inputs, seed and draw
// give the same bits.  The box arithmetic relies on -ffp-contract=off (csrc/Makefile): no product is fused into a sum.
#include "sampler.h"

#include <cmath>

#include "philox.h"

namespace mpn {

constexpr int kAttachThreads = 256;   // rows per block, and boxes per LDS tile
constexpr int kSampleThreads = 1024;  // the sampler's one block: 16 waves
constexpr int kMaxRecordRows = 1 << 28;

// One thread per row of all_boxes = [gt ; proposals].  The GT boxes with their labels, then the crowd boxes, pass through LDS in tiles of
// kAttachThreads boxes (every thread of the block stages one box, rows past m included), so g and n_crowd have no limit.
//   utils.boxoverlap (utils.lua:104-128) in fp32: w = x2 - x1 + 1, h = y2 - y1 + 1, inter = w * h, o = inter / (aarea + barea - inter),
//   0 where w < 0 or h < 0; the maximum over the GT boxes in order and the FIRST maximum's 1-based index (strict >), 0 where the maximum is 0.
//   utils.intersection (utils.lua:131-148): inter / aarea WITHOUT the zeroing — a box off a crowd's corner (w < 0 and h < 0) has a positive
//   inter; the reference's property, kept.  Rows >= g whose maximum over the crowds is > 0.7f get overlap = -1;
//   correspondance and label stay as they are (DataSetJSON.lua:345-371).
__global__ __launch_bounds__(kAttachThreads) void attach_proposals_kernel(const float *__restrict__ prop, int n, const float *__restrict__ gt,
                                                                          const int *__restrict__ gt_labels, int g, const float *__restrict__ crowds,
                                                                          int n_crowd, float *__restrict__ boxes, float *__restrict__ overlap,
                                                                          int *__restrict__ corr, int *__restrict__ label) {
  __shared__ float tile[kAttachThreads][4];
  __shared__ int tile_label[kAttachThreads];
  const int m = g + n, tid = threadIdx.x;
  const int i = blockIdx.x * kAttachThreads + tid;
  const bool live = i < m;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (live) {
    const float *src = i < g ? gt + 4 * (size_t)i : prop + 4 * (size_t)(i - g);
    a0 = src[0]; a1 = src[1]; a2 = src[2]; a3 = src[3];
  }
  const float aarea = (a2 - a0 + 1.0f) * (a3 - a1 + 1.0f);
  float best = 0.0f;
  int best_j = 0, best_label = 0;
  for (int j0 = 0; j0 < g; j0 += kAttachThreads) {
    const int cnt = min(kAttachThreads, g - j0);
    if (tid < cnt) {
      const float *b = gt + 4 * (size_t)(j0 + tid);
      tile[tid][0] = b[0]; tile[tid][1] = b[1]; tile[tid][2] = b[2]; tile[tid][3] = b[3];
      tile_label[tid] = gt_labels[j0 + tid];
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const float b0 = tile[j][0], b1 = tile[j][1], b2 = tile[j][2], b3 = tile[j][3];
      const float x1 = a0 < b0 ? b0 : a0, y1 = a1 < b1 ? b1 : a1, x2 = a2 > b2 ? b2 : a2, y2 = a3 > b3 ? b3 : a3;
      const float w = x2 - x1 + 1.0f, h = y2 - y1 + 1.0f, inter = w * h;
      const float barea = (b2 - b0 + 1.0f) * (b3 - b1 + 1.0f);
      float o = inter / (aarea + barea - inter);
      if (w < 0.0f || h < 0.0f) o = 0.0f;
      if (j0 + j == 0 || o > best) { best = o; best_j = j0 + j + 1; best_label = tile_label[j]; }
    }
    __syncthreads();
  }
  if (best == 0.0f) { best_j = 0; best_label = 0; }
  bool masked = false;
  float cmax = 0.0f;
  for (int j0 = 0; j0 < n_crowd; j0 += kAttachThreads) {
    const int cnt = min(kAttachThreads, n_crowd - j0);
    if (tid < cnt) {
      const float *b = crowds + 4 * (size_t)(j0 + tid);
      tile[tid][0] = b[0]; tile[tid][1] = b[1]; tile[tid][2] = b[2]; tile[tid][3] = b[3];
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const float b0 = tile[j][0], b1 = tile[j][1], b2 = tile[j][2], b3 = tile[j][3];
      const float x1 = a0 < b0 ? b0 : a0, y1 = a1 < b1 ? b1 : a1, x2 = a2 > b2 ? b2 : a2, y2 = a3 > b3 ? b3 : a3;
      const float w = x2 - x1 + 1.0f, h = y2 - y1 + 1.0f, inter = w * h;
      const float r = inter / aarea;
      if (j0 + j == 0 || r > cmax) cmax = r;
    }
    __syncthreads();
  }
  if (n_crowd > 0 && i >= g && cmax > 0.7f) masked = true;
  if (!live) return;
  float *o = boxes + 4 * (size_t)i;
  o[0] = a0; o[1] = a1; o[2] = a2; o[3] = a3;
  overlap[i] = masked ? -1.0f : best;
  corr[i] = best_j;
  label[i] = best_label;
}

struct RoiSampleArgs {
  const float *boxes, *overlap;
  const int *corr, *label;
  int m, bg_num, fg_num, flip;
  float fg_thr, bg_lo, bg_hi, im_w;
  uint32_t seed_lo, seed_hi, draw_lo, draw_hi;
  int *list_bg, *list_fg;   // [m] each
  float *rois, *gt;
  int *labels, *counts;
};

// ONE block.  (a) the two row lists in ascending order, as nonzero() returns them (setupOne): per chunk of kSampleThreads rows a wave
// ballot per set gives every lane its rank inside the wave, the 16 waves' counts go through LDS and each thread adds those of the waves
// before its own to the running total.  (b) min(num, count) draws WITH replacement per set: draw i of set s (0 background, 1 foreground)
// is word 0 of Philox4x32-10(counter = (i, draw_lo, 0x80000000 + s, draw_hi), key = (seed_lo, seed_hi)) mapped to
// (uint64(word) * count) >> 32 — the high bit of counter word 2 keeps the stream apart from the dropout masks' (layer < 2^31) under the
// same seed.  (c) the gather: background rows first, then foreground (BatchProviderROI.lua:98-101); gt = zeros / the GT box the row
// corresponds to; flip: both tables through utils.flipBoxes at width im_w.  Nothing past row r_bg + r_fg is written.
__global__ __launch_bounds__(kSampleThreads) void roi_sample_kernel(RoiSampleArgs a) {
  __shared__ int wsum[2][kSampleThreads / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const unsigned long long below = (1ull << lane) - 1ull;
  int n_bg = 0, n_fg = 0;
  for (int base = 0; base < a.m; base += kSampleThreads) {
    const int i = base + tid;
    bool fg = false, bg = false;
    if (i < a.m) {
      const float ov = a.overlap[i];
      fg = ov >= a.fg_thr;
      bg = ov >= a.bg_lo && ov < a.bg_hi;
    }
    const unsigned long long mb = __ballot(bg), mf = __ballot(fg);
    if (lane == 0) { wsum[0][wave] = __popcll(mb); wsum[1][wave] = __popcll(mf); }
    __syncthreads();
    int ob = n_bg, of = n_fg;
    for (int w = 0; w < kSampleThreads / kWave; ++w) {
      const int cb = wsum[0][w], cf = wsum[1][w];
      if (w < wave) { ob += cb; of += cf; }
      n_bg += cb; n_fg += cf;
    }
    if (bg) a.list_bg[ob + __popcll(mb & below)] = i;
    if (fg) a.list_fg[of + __popcll(mf & below)] = i;
    __syncthreads();  // wsum is rewritten by the next chunk; after the last one the lists are visible to the whole block
  }
  if (tid == 0) { a.counts[0] = n_bg; a.counts[1] = n_fg; }
  const int r_bg = min(a.bg_num, n_bg), r_fg = min(a.fg_num, n_fg);
  for (int t = tid; t < r_bg + r_fg; t += kSampleThreads) {
    const int s = t >= r_bg ? 1 : 0, i = s ? t - r_bg : t, count = s ? n_fg : n_bg;
    uint32_t w[4];
    philox4x32_10((uint32_t)i, a.draw_lo, 0x80000000u + (uint32_t)s, a.draw_hi, a.seed_lo, a.seed_hi, w);
    const int pick = (int)(((uint64_t)w[0] * (uint64_t)count) >> 32);   // < count
    const int row = (s ? a.list_fg : a.list_bg)[pick];
    const float *b = a.boxes + 4 * (size_t)row;
    float r0 = b[0], r1 = b[1], r2 = b[2], r3 = b[3];
    float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f, g3 = 0.0f;
    int lab = 0;
    if (s) {
      const int c = a.corr[row];
      if (c >= 1 && c <= a.m) {  // (a foreground row has overlap >= fg_thr > 0, so a GT box; with fg_thr <= 0 a row without one keeps zeros)
        const float *q = a.boxes + 4 * (size_t)(c - 1);
        g0 = q[0]; g1 = q[1]; g2 = q[2]; g3 = q[3];
      }
      lab = a.label[row];
    }
    if (a.flip) {
      const float f0 = flip_x(r2, a.im_w), f2 = flip_x(r0, a.im_w), h0 = flip_x(g2, a.im_w), h2 = flip_x(g0, a.im_w);
      r0 = f0; r2 = f2; g0 = h0; g2 = h2;
    }
    float *ro = a.rois + 4 * (size_t)t, *go = a.gt + 4 * (size_t)t;
    ro[0] = r0; ro[1] = r1; ro[2] = r2; ro[3] = r3;
    go[0] = g0; go[1] = g1; go[2] = g2; go[3] = g3;
    a.labels[t] = lab;
  }
}

int check_attach_args(const char *fn, const float *d_proposals, int n, const float *d_gt, const int *d_gt_labels, int g, const float *d_crowds,
                      int n_crowd) {
  const char *bad = nullptr;
  if (n < 0) bad = "n < 0";
  else if (g < 0) bad = "g < 0";
  else if (n_crowd < 0) bad = "n_crowd < 0";
  else if (g == 0 && n == 0) bad = "g + n == 0: no rows";
  else if ((long long)g + n > kMaxRecordRows) bad = "g + n exceeds 2^28 rows";
  else if (n > 0 && !d_proposals) bad = "d_proposals is NULL with n > 0";
  else if (g > 0 && !d_gt) bad = "d_gt is NULL with g > 0";
  else if (g > 0 && !d_gt_labels) bad = "d_gt_labels is NULL with g > 0";
  else if (n_crowd > 0 && !d_crowds) bad = "d_crowds is NULL with n_crowd > 0";
  if (!bad) return MPN_OK;
  set_error("%s: invalid argument: %s", fn, bad);
  return MPN_EINVAL;
}

int check_sampler_cfg(const char *fn, const mpn_roi_sampler *cfg, int flip_width) {
  const char *bad = nullptr;
  if (!cfg) bad = "cfg is NULL";
  else if (cfg->batch_size <= 0) bad = "cfg->batch_size <= 0";
  else if (!std::isfinite(cfg->fg_fraction) || cfg->fg_fraction < 0.0 || cfg->fg_fraction > 1.0) bad = "cfg->fg_fraction is not a finite number in [0, 1]";
  else if (!std::isfinite(cfg->fg_threshold)) bad = "cfg->fg_threshold is not finite";
  else if (!std::isfinite(cfg->bg_lo) || !std::isfinite(cfg->bg_hi)) bad = "cfg->bg_lo / cfg->bg_hi is not finite";
  else if (cfg->bg_lo > cfg->bg_hi) bad = "cfg->bg_lo > cfg->bg_hi";
  else if (flip_width < 0) bad = "flip_width < 0";
  if (!bad) return MPN_OK;
  set_error("%s: invalid argument: %s", fn, bad);
  return MPN_EINVAL;
}

int attach_proposals(const float *d_proposals, int n, const float *d_gt, const int *d_gt_labels, int g, const float *d_crowds, int n_crowd,
                     float *d_boxes, float *d_overlap, int *d_corr, int *d_label, hipStream_t s) {
  hipLaunchKernelGGL(attach_proposals_kernel, dim3((unsigned)cdiv(g + n, kAttachThreads)), dim3(kAttachThreads), 0, s, d_proposals, n, d_gt,
                     d_gt_labels, g, d_crowds, n_crowd, d_boxes, d_overlap, d_corr, d_label);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

int roi_sample(const float *d_boxes, const float *d_overlap, const int *d_corr, const int *d_label, int m, const mpn_roi_sampler &cfg,
               uint64_t seed, uint64_t draw, int flip_width, int *d_lists, float *d_rois, float *d_gt, int *d_labels, int *d_counts, hipStream_t s) {
  RoiSampleArgs a{};
  a.boxes = d_boxes; a.overlap = d_overlap; a.corr = d_corr; a.label = d_label; a.m = m;
  a.fg_num = sampler_fg_num(cfg); a.bg_num = cfg.batch_size - a.fg_num;
  a.flip = flip_width > 0 ? 1 : 0; a.im_w = (float)flip_width;
  a.fg_thr = cfg.fg_threshold; a.bg_lo = cfg.bg_lo; a.bg_hi = cfg.bg_hi;
  a.seed_lo = (uint32_t)(seed & 0xffffffffu); a.seed_hi = (uint32_t)(seed >> 32);
  a.draw_lo = (uint32_t)(draw & 0xffffffffu); a.draw_hi = (uint32_t)(draw >> 32);
  a.list_bg = d_lists; a.list_fg = d_lists + m;
  a.rois = d_rois; a.gt = d_gt; a.labels = d_labels; a.counts = d_counts;
  hipLaunchKernelGGL(roi_sample_kernel, dim3(1), dim3(kSampleThreads), 0, s, a);
  MPN_CHECK_LAUNCH();
  return MPN_OK;
}

}  // namespace mpn

using namespace mpn;

extern "C" int mpn_attach_proposals(const float *d_proposals, int n, const float *d_gt, const int *d_gt_labels, int g, const float *d_crowds,
                                    int n_crowd, float *d_boxes, float *d_overlap, int *d_corr, int *d_label, void *stream) {
  int rc = check_attach_args("mpn_attach_proposals", d_proposals, n, d_gt, d_gt_labels, g, d_crowds, n_crowd);
  if (rc) return rc;
  MPN_CHECK_ARG(d_boxes && d_overlap && d_corr && d_label);
  return attach_proposals(d_proposals, n, d_gt, d_gt_labels, g, d_crowds, n_crowd, d_boxes, d_overlap, d_corr, d_label, as_stream(stream));
}

extern "C" int mpn_sample_rois(const float *d_boxes, const float *d_overlap, const int *d_corr, const int *d_label, int m,
                               const mpn_roi_sampler *cfg, uint64_t seed, uint64_t draw, int flip_width, float *d_rois, float *d_gt,
                               int *d_labels, int *d_counts, void *stream) {
  int rc = check_sampler_cfg("mpn_sample_rois", cfg, flip_width);
  if (rc) return rc;
  MPN_CHECK_ARG(d_boxes && d_overlap && d_corr && d_label && d_rois && d_gt && d_labels && d_counts);
  MPN_CHECK_ARG(m > 0 && m <= kMaxRecordRows);
  hipStream_t s = as_stream(stream);
  void *lists = nullptr;
  rc = scratch_get(SCR_MISC, 2 * (size_t)m * sizeof(int), s, &lists);
  if (rc) return rc;
  return roi_sample(d_boxes, d_overlap, d_corr, d_label, m, *cfg, seed, draw, flip_width, static_cast<int *>(lists), d_rois, d_gt, d_labels,
                    d_counts, s);
}
