/* mpn.h — C ABI of libmpn_hip.so: the MI355X (gfx950) per-image detection hot path of MultiPathNet.
 *
 * Drop-in boundary.  Every entry point mirrors ONE reference surface — an
 * nn.Module:updateOutput, a utils.lua helper, or an nms.c export — and cites it.  Plain pointers and
 * sizes only; no torch / TH types.  (The TH-struct-compatible `NMS` / `bbox_vote` pair that
 * utils.lua:15-19 binds lives in include/mpn_libnms.h → libnms.so.)
 *
 * Conventions
 *   - `d_` pointers are DEVICE (HBM) pointers on the current HIP device, fp32, contiguous, row-major,
 *     Torch layout (NCHW images/features, [N,5] rois = {batch(1-based), x1,y1,x2,y2} 1-based pixels).
 *   - `h_` pointers are host pointers.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls enqueue work and
 *     return; they never synchronise unless the name ends in `_host` / `_sync`.
 *   - Return value: MPN_OK or a negative mpn_status; mpn_last_error() gives a thread-local message.
 *     Nothing aborts.  Module-level calls allocate only what a `ws` (workspace) argument documents, plus the shared
 *     scratch named under Concurrency; pipeline handles allocate everything at creation.
 *   - Concurrency: re-entrant.  The reference host runs one worker thread per GPU inside ONE process
 *     (test_runner.lua:55-66: Threads(nGPU) + cutorch.setDevice per thread); this library has no process-global device
 *     state.  A pipeline handle (mpn_frcnn) owns every buffer it uses, including its split-K / NMS scratch, and lives on
 *     the device that was current at creation: drive ONE handle from one thread at a time (with that device current);
 *     different handles — same or different devices — may run concurrently from different host threads and streams.
 *     Module-level calls keep their grow-on-demand scratch per (device, stream) pair, so calls on different streams
 *     or devices never share it either — but ONE thread at a time per (device, stream): two host threads issuing
 *     module-level calls on the same stream (the NULL stream included) would grow and use one scratch concurrently.
 *     A host that creates streams per image releases a stream's scratch with mpn_stream_release before it destroys
 *     the stream (tens of MB of NMS masks per entry otherwise stay until mpn_release_all_scratch / process exit).
 *   - Integer results (argmax, keep indices, counts) are bit-exact vs the reference semantics; fp32
 *     box arithmetic is evaluated without FMA contraction, in the reference's operation order.
 */
#ifndef MPN_H
#define MPN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPN_VERSION 600

typedef enum mpn_status {
  MPN_OK = 0,
  MPN_EINVAL = -1,   /* bad argument (null pointer, non-positive size, unsupported shape) */
  MPN_EHIP = -2,     /* a HIP runtime call or kernel launch failed */
  MPN_ENOMEM = -3,   /* workspace too small / allocation failed */
  MPN_ENCCL = -4,    /* an RCCL call failed (mpn_comm_*, mpn_gather_dets) */
  MPN_ESTATE = -5    /* object used in the wrong state */
} mpn_status;

int mpn_version(void);
const char *mpn_last_error(void);
/* Fills name[] with the device's gcnArchName; returns MPN_EHIP when no HIP device is usable. */
int mpn_device_info(char *name, int name_len, int *cu_count, size_t *hbm_bytes);
/* Frees the module-level scratch kept for (current device, stream) after synchronising that stream; call it before
 * hipStreamDestroy when streams come and go.  mpn_release_all_scratch does it for every (device, stream) entry (the host
 * must have quiesced all module-level work).  Pipeline handles are unaffected: their scratch dies with the handle. */
int mpn_stream_release(void *stream);
int mpn_release_all_scratch(void);

/* ------------------------------------------------------------------------------------------------
 * NMS family — replaces nms.c (the reference's only native code)
 * ---------------------------------------------------------------------------------------------- */

/* nms.c:59-108 `NMS`, batched over classes (Tester_FRCNN.lua:106-125 calls it once per class).
 *   d_scored [n_cls, m_stride, 5] {x1,y1,x2,y2,score}; class c has d_counts[c] valid rows
 *   (d_counts == NULL -> every class has m_stride rows).
 *   d_keep      [n_cls, m_stride, 5]  kept rows in SELECTION order (as nms.c:102-105 writes them)
 *   d_keep_idx  [n_cls, m_stride]     original row index of each kept box (may be NULL)
 *   d_n_keep    [n_cls]               number kept
 * Greedy selection, IoU with the +1 convention (nms.c:14-41), suppression when IoU > thr,
 * tie-breaking among bit-equal scores identical to nms.c:74-98 (swap + stable partition history).
 * Tables of up to 1024 rows per class take ONE launch (sort, suppression mask sliced over the GPU, greedy selection with the exact position
 * rule in one CU's LDS); tables up to MPN_NMS_MAX_BOXES rows a chain of launches (bitonic sort -> suppression bitmask -> wave scan; also
 * what the pipelined mpn_frcnn_* forms run above 384 rows, their NMS sharing the GPU with the next image's trunk);
 * wider tables are accepted too (nms.c has no size limit) and take the exact sweep kernel on HBM-resident arrays. */
#define MPN_NMS_MAX_BOXES 6144
int mpn_nms_batched(const float *d_scored, const int *d_counts, int n_cls, int m_stride, float thr, float *d_keep,
                    int *d_keep_idx, int *d_n_keep, void *stream);

/* Single-class convenience (== utils.nms, utils.lua:29-33) on device buffers. */
int mpn_nms(const float *d_scored, int m, float thr, float *d_keep, int *d_keep_idx, int *d_n_keep, void *stream);

/* utils.nms_dense (utils.lua:402-462, called by demo.lua:85): the index-returning NMS — sort by score (descending), walk the
 * sorted list, a picked box suppresses every box whose IoU with it (areas with the +1 convention, intersection clamped at 0)
 * exceeds `overlap` (strict).  d_boxes [m,5] {x1,y1,x2,y2,score}; d_pick [m] int32 receives the picks as 1-BASED row indices
 * in pick order (the LongTensor the Lua function returns), *d_n_pick their number.  Any m (tables wider than the 8192 rows the
 * LDS sort holds take a counting-rank + sequential-walk form: the reference function has no size limit).  The order among
 * bit-equal scores is the sort's: torch.sort is TH's (unstable) quicksort and TH is absent from the reference tree — PARITY
 * UNPINNED there; this library sorts ties by ascending index, NaN scores last. */
int mpn_nms_dense(const float *d_boxes, int m, float overlap, int *d_pick, int *d_n_pick, void *stream);

/* Host-buffer form used by the libnms.so drop-in, synchronous.  h_keep [m,5].  Tables of up to 1024 rows are staged in a per-thread pinned,
 * device-mapped buffer that the kernel reads and writes directly (no device allocation, no hipMemcpy: one launch + one stream sync);
 * wider ones go H2D -> kernels -> D2H. */
int mpn_nms_host(const float *h_scored, int m, float thr, float *h_keep, int *h_keep_idx, int *n_keep);

/* nms.c:110-142 `bbox_vote`: d_res[i] = score-weighted mean of all scored boxes with IoU(j,i) > thr
 * (strict), accumulated sequentially in j order; d_res[i][4] = nms score.  d_nms [n_nms,5],
 * d_scored [m,5], d_res [n_nms,5].  d_n_nms (device int, may be NULL) overrides n_nms at run time. */
int mpn_bbox_vote(const float *d_nms, int n_nms, const int *d_n_nms, const float *d_scored, int m, float thr,
                  float *d_res, void *stream);
/* The per-class voting loop of Tester_FRCNN.lua:118-124 in one launch: class c votes d_keep[c] (n_keep[c] rows) against
 * d_scored[c] (counts[c] rows) with weights score^score_pow (opt.test_bbox_voting_score_pow; 1 = nms.c arithmetic exactly). */
int mpn_bbox_vote_batched(const float *d_keep, const int *d_n_keep, const float *d_scored, const int *d_counts, int n_cls,
                          int m_stride, float thr, float score_pow, float *d_res, void *stream);
int mpn_bbox_vote_host(const float *h_nms, int n_nms, const float *h_scored, int m, float thr, float *h_res);

/* nms.c:43-56 `boxoverlap`: IoU of n boxes [n,4] against one box (h_b[4], host). */
int mpn_boxoverlap(const float *d_a, int n, const float *h_b, float *d_out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Image / ROI preparation — ImageTransformer.lua, ImageDetect.lua
 * ---------------------------------------------------------------------------------------------- */

/* fbcoco.ImageTransformer:updateOutput (modules/ImageTransformer.lua:19-33):
 * out[i] = (in[swap[i]]*scale - mean[i]) / std[i], f64 arithmetic rounded once to fp32
 * (the reference transforms a DoubleTensor, ImageDetect.lua:29,44-50).  swap is 0-based;
 * h_std == NULL skips the division.  d_in, d_out [3,H,W]. */
int mpn_image_transform(const float *d_in, int H, int W, const int *h_swap, double scale, const double *h_mean,
                        const double *h_std, float *d_out, void *stream);

/* image.scale(src, W2, H2) in its default bilinear mode (external `image` rock; ImageDetect.lua:41).  PARITY
 * UNPINNED: restated from torch/image's published separable algorithm — rows then columns through a float
 * intermediate; upscaling interpolates with i+f = d*(src-1)/(dst-1) (last sample copied), downscaling is a
 * fractional box average over [d*s,(d+1)*s), s = src/dst.  d_in [C,H,W] -> d_out [C,H2,W2]; d_tmp holds C*H*W2 floats.
 * ImageDetect.lua:40 sizes the output as (long)(H*scale) x (long)(W*scale). */
int mpn_image_scale(const float *d_in, int C, int H, int W, int H2, int W2, float *d_tmp, float *d_out, void *stream);

/* ImageDetect.lua:34-43: scale factor for one image (host arithmetic). */
double mpn_pick_scale(int H, int W, double target, double max_size);

/* project_im_rois (ImageDetect.lua:66-70): rois = {1, (boxes-1)*s+1}.  d_boxes [n,4] -> d_rois [n,5]. */
int mpn_project_im_rois(const float *d_boxes, int n, double scale, float *d_rois, void *stream);

/* project_im_rois' multi-scale branch (ImageDetect.lua:57-65), completed as Fast R-CNN's _project_im_rois does.
 * In fp32, each operation rounded: w = x2 - x1 + 1, h = y2 - y1 + 1, area = w*h, d_l = |area * (s_l*s_l) - 224*224| with
 * s_l = (float)h_scales[l]; level = the FIRST l with minimal d_l under TH's min (a NaN difference stops the scan where it stands, so
 * boxes whose differences are all equal or all NaN land on level 0).  d_rois [n,5] = {level + 1, (x1-1)*s_level+1, ...}: column 0
 * is inn.ROIPooling's 1-based batch index into the [S,C,h,w] stack of level maps.  1 <= n_scales <= MPN_MAX_SCALES, every scale
 * finite and > 0.  n_scales == 1 is mpn_project_im_rois bit for bit. */
#define MPN_MAX_SCALES 8
int mpn_project_im_rois_levels(const float *d_boxes, int n, int n_scales, const double *h_scales, float *d_rois, void *stream);

/* image.hflip (BatchProviderBase.lua:22): d_out[c,y,x] = d_in[c,y,W-1-x].  d_in, d_out [C,H,W], d_in != d_out. */
int mpn_image_hflip(const float *d_in, int C, int H, int W, float *d_out, void *stream);

/* utils.flipBoxes (utils.lua:151-155): x1' = ((-x2) + image_width) + 1, x2' = ((-x1) + image_width) + 1 in fp32, each operation
 * rounded on its own (no FMA), y unchanged.  d_boxes, d_out [n,4]; d_out may be d_boxes.  An involution on integer-valued
 * coordinates below 2^24; not on others. */
int mpn_flip_boxes(const float *d_boxes, int n, int image_width, float *d_out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * nn.Module:updateOutput mirrors
 * ---------------------------------------------------------------------------------------------- */

/* inn.ROIPooling(PW,PH,scale):updateOutput{feat, rois} (vgg.lua:28, alexnet.lua:23, resnet.lua:48,
 * inceptionv3.lua:41, model_utils.lua:215).  d_feat [B,C,H,W], d_rois [N,5] -> d_out [N,C,PH,PW],
 * d_argmax [N,C,PH,PW] int32 (h*W+w within the plane, -1 for an empty bin; may be NULL).
 * start=round((x1-coord_offset)*scale), end=round((x2-coord_offset)*scale)+end_adjust, ROI forced
 * >= 1x1, bins floor/ceil of fp32 bin size, clipped to the map, empty bin -> 0.
 * Reference default ("v2" fix, README.md:202-203): coord_offset=1, end_adjust=0. */
/* inn.ROIPooling:updateGradInput: d_grad_in [B,C,H,W] from d_grad_out [N,C,PH,PW] and the argmax mpn_roi_pool_forward wrote
 * (column 0 of d_rois [N,5] is the 1-based map index, clamped as the forward clamps it).  Every cell is written:
 *   grad_in[b,c,y,x] = sum of grad_out[n,c,bin] over the rows n of map b ASCENDING and, inside a row, the bins ascending
 *   (ph * PW + pw), wherever argmax[n,c,bin] == y * W + x — fp32 adds from +0.0, no atomics: the order is part of the contract. */
int mpn_roi_pool_backward(const float *d_grad_out, const int32_t *d_argmax, const float *d_rois, int B, int C, int H, int W, int N,
                          int PH, int PW, float *d_grad_in, void *stream);
int mpn_roi_pool_forward(const float *d_feat, int B, int C, int H, int W, const float *d_rois, int N, int PH, int PW,
                         float scale, float coord_offset, int end_adjust, float *d_out, int32_t *d_argmax,
                         void *stream);
/* The same module with an explicit BIN RULE (inn.ROIPooling is external and its source is not in the reference tree: both of its branches are
 * restated, SURVEY §8a-6, parity unpinned):
 *   MPN_ROI_BINS_CAFFE    — the CUDA branch (what mpn_roi_pool_forward computes): bins from the un-clipped window, each bin clipped to the map
 *                           afterwards, a bin that falls outside the map is empty (0, argmax -1);
 *   MPN_ROI_BINS_ADAPTIVE — the CPU branch ("CPU nn path", BASELINE configs[0]; call sites models/alexnet.lua:23, models/vgg.lua:28 with float
 *                           tensors): corners = round((x - coord_offset) * scale + 1) in 1-based map coordinates, CLIPPED to the map first
 *                           (the reference clips the upper side — cmin — and indexes the tensor with the lower side; we clip both), the crop
 *                           goes through nn.SpatialAdaptiveMaxPooling(PW, PH): bin p = [floor(p * size / P), ceil((p + 1) * size / P)) of the
 *                           clipped crop, never empty.  The two rules differ on windows whose rounded corners leave the map (Foveal's regions; border boxes whose
 *                           round((x2 - 1) * scale) is W) and, about once in a thousand windows, by one cell where the fp32 bin size rounds
 *                           (measured: tests/test_oracle_roipool_adaptive.py).
 * d_argmax is h * W + w in the feature plane under both rules. */
#define MPN_ROI_BINS_CAFFE 0
#define MPN_ROI_BINS_ADAPTIVE 1
int mpn_roi_pool_forward_rule(const float *d_feat, int B, int C, int H, int W, const float *d_rois, int N, int PH, int PW,
                              float scale, float coord_offset, int end_adjust, int bin_rule, float *d_out, int32_t *d_argmax,
                              void *stream);

/* nn.Foveal:updateOutput (modules/Foveal.lua:15-44): [N,5] -> [4N,5], f64 arithmetic rounded to fp32. */
int mpn_foveal_forward(const float *d_rois, int N, float *d_out, void *stream);

/* nn.ContextRegion(scale):updateOutput (modules/ContextRegion.lua:14-32): [N,5] -> [N,5]. */
int mpn_context_region_forward(const float *d_rois, int N, double scale, float *d_out, void *stream);

/* nn.BBoxNorm:updateOutput, evaluate mode (modules/BBoxNorm.lua:18-32): in place, view(-1,4)*std+mean. */
int mpn_bbox_norm_forward(float *d_bbox, int N, int C4, const float *h_mean4, const float *h_std4, void *stream);

/* nn.SelectBoxes:updateOutput (modules/SelectBoxes.lua:26-56): first arg-max class -> its 4 coords. */
int mpn_select_boxes_forward(const float *d_scores, const float *d_bbox, int N, int C, float *d_out, void *stream);

/* nn.SoftMax:updateOutput over dim 2 (ImageDetect.lua:19,189-191).  [M,C] -> [M,C]. */
int mpn_softmax_forward(const float *d_x, int M, int C, float *d_y, void *stream);

/* cudnn.SpatialConvolution(Cin,Cout,3,3,1,1,1,1):updateOutput (+ fused nn.ReLU) as in `features`
 * (models/vgg.lua:15,25; multipathnet.lua:34-46).  NCHW in/out, d_w [Cout,Cin,3,3], d_b [Cout] or NULL.
 * fp32 MFMA implicit GEMM.  The activations are converted to the library's channel-blocked HBM layout
 * inside `ws`; mpn_conv3x3_workspace_bytes gives the size needed. */
size_t mpn_conv3x3_workspace_bytes(int B, int Cin, int H, int W, int Cout);
/* nn.SpatialConvolution:updateGradInput + accGradParameters of the module mpn_conv3x3_forward mirrors (no fused ReLU: d_grad_out is the
 * gradient at the convolution's output), NCHW in and out:
 *   d_grad_in [B,Cin,H,W]   = conv3x3(d_grad_out, W rotated by 180 degrees with cin / cout swapped)   (needs d_w)
 *   d_grad_w  [Cout,Cin,3,3] = sum over the B maps, in order, of sum_{y,x} grad_out[co,y,x] in[ci,y+ky-1,x+kx-1]   (needs d_in)
 *   d_grad_b  [Cout]         = sum over the maps and pixels of grad_out
 * Each of the three may be NULL; gradients are OVERWRITTEN, not accumulated.  The same kernels as the training pipeline
 * (mpn_frcnn_train_step at depth MPN_TRAIN_CONV(k)): fixed summation orders, no atomics — the same bits in every run.  Workspace and
 * stream conventions of mpn_conv3x3_forward; mpn_conv3x3_backward_workspace_bytes gives the size. */
size_t mpn_conv3x3_backward_workspace_bytes(int B, int Cin, int H, int W, int Cout);
int mpn_conv3x3_backward(const float *d_in, int B, int Cin, int H, int W, const float *d_w, const float *d_grad_out, int Cout,
                         float *d_grad_in, float *d_grad_w, float *d_grad_b, void *ws, size_t ws_bytes, void *stream);
int mpn_conv3x3_forward(const float *d_in, int B, int Cin, int H, int W, const float *d_w, const float *d_b,
                        int Cout, int relu, float *d_out, void *d_ws, size_t ws_bytes, void *stream);

/* nn.SpatialMaxPooling(2,2,2,2):ceil():updateOutput.  [B*C,H,W] -> [B*C,ceil(H/2),ceil(W/2)]. */
int mpn_maxpool2x2_ceil_forward(const float *d_in, int BC, int H, int W, float *d_out, void *stream);
/* nn.SpatialMaxPooling(2,2,2,2):ceil():updateGradInput.  d_in [B*C,H,W] the forward's input, d_grad_out [B*C,ceil(H/2),ceil(W/2)],
 * d_grad_in [B*C,H,W].  Windows do not overlap, so every input cell belongs to exactly one window (Y, X) = (y / 2, x / 2):
 *   d_grad_in[c,y,x] = d_grad_out[c,Y,X]  if (y, x) is the cell on which the forward's scan of the window ends — the scan starts from
 *                                         -inf, tests v > m and visits (2Y,2X), (2Y,2X+1), (2Y+1,2X), (2Y+1,2X+1), skipping cells outside
 *                                         the map: the FIRST maximum in row-major order wins, a window holding only NaN routes nowhere;
 *                      +0.0               everywhere else.
 * Pure routing: no additions, no atomics, every cell of d_grad_in written exactly once — bit-exact by construction.  The maxima are
 * recomputed from d_in (no argmax plane, no pooled map).  relu_mask != 0 is the form the training pipeline uses, fused with the ReLU
 * of the layer the gradient flows into: a cell also gets +0.0 where d_in <= 0 (d_in post-ReLU: an all-zero window routes nothing). */
int mpn_maxpool2x2_ceil_backward(const float *d_in, const float *d_grad_out, int BC, int H, int W, int relu_mask, float *d_grad_in,
                                 void *stream);

/* nn.Linear(K,N):updateOutput (+ fused nn.ReLU) (vgg.lua:16,30 `top`; model_utils.lua:105-119).
 * y[M,N] = x[M,K] W[N,K]^T + b.  fp32 MFMA; per-output k-ascending fmaf chain, independent of M
 * (so chunked == un-chunked exactly, test.lua:140-179). */
int mpn_linear_forward(const float *d_x, int M, int K, const float *d_w, const float *d_b, int N, int relu,
                       float *d_y, void *stream);

/* ------------------------------------------------------------------------------------------------
 * utils.lua / Tester_FRCNN.lua helpers
 * ---------------------------------------------------------------------------------------------- */

/* utils.convertFrom, 2-D path, for every 4-column class block (utils.lua:229-247,
 * ImageDetect.lua:183-185).  d_boxes [N,4] original-image boxes, d_deltas [N,4C] -> d_out [N,4C].
 * Alignment: the kernel moves whole 4-vectors, so d_boxes, d_deltas and d_out must each be 16-byte aligned (any
 * hipMalloc'd base is; a view that starts at a row of a contiguous table is too, one that starts inside a row may not
 * be).  A pointer that is not is refused with MPN_EINVAL and a message naming the argument; nothing is launched. */
int mpn_bbox_decode(const float *d_boxes, const float *d_deltas, int N, int C, float *d_out, void *stream);

/* Tester_FRCNN.lua:75-78: in place, x -> [1,im_w], y -> [1,im_h] on the (x,y) pairs of d_bbox.  A NaN stays a NaN.
 * Alignment: d_bbox must be 8-byte aligned (the kernel moves whole pairs); otherwise MPN_EINVAL naming it, nothing launched. */
int mpn_clamp_boxes(float *d_bbox, size_t n_pairs, float im_w, float im_h, void *stream);

/* Tester_FRCNN.lua:106-116 for all classes j = first_cls .. C-1 at once: rows with score > thresh,
 * in row order -> d_scored [C-first_cls, N, 5], d_counts [C-first_cls], d_src_idx (may be NULL).  A NaN score is not
 * greater than any threshold: its row is dropped.  Rows of d_scored beyond d_counts[c] are not written.
 * Alignment: d_bbox [N,4C] must be 16-byte aligned (each class's 4-vector is read whole); otherwise MPN_EINVAL naming
 * it, nothing launched.  d_scores and d_scored (5-float rows) need only their natural 4 bytes. */
int mpn_select_scored(const float *d_scores, const float *d_bbox, int N, int C, int first_cls, float thresh,
                      float *d_scored, int *d_counts, int *d_src_idx, void *stream);

/* utils.keep_top_k (utils.lua:75-96): threshold = k-th largest kept score over all classes (ties
 * survive).  d_keep [n_cls, m_stride, 5] / d_n_keep [n_cls] as written by mpn_nms_batched.
 * Writes *d_thresh (device float) and compacts survivors into d_out [max_out, 6] =
 * {x1,y1,x2,y2,score,class(1-based, as float)} class-major.  *d_n_out receives the UNTRUNCATED number of survivors:
 * when it exceeds max_out (many ties at the threshold), only the first max_out rows were written and the caller
 * knows rows were dropped (utils.keep_top_k itself never truncates).
 * Arguments: k >= 1, 0 <= n_cls <= 1024, m_stride >= 0, max_out >= 0; anything else answers MPN_EINVAL and launches nothing
 * (both entries).  Counts above m_stride are read as m_stride, negative counts as 0.  -0.0f and 0.0f are one score.  NaN scores
 * are not supported: utils.keep_top_k sorts them with a comparison that gives no defined order. */
int mpn_keep_top_k(const float *d_keep, const int *d_n_keep, int n_cls, int m_stride, int k, float *d_thresh,
                   float *d_out, int max_out, int *d_n_out, void *stream);
/* The same on tables whose rows are in NON-INCREASING score order inside every class — what mpn_nms_batched emits (each greedy round picks the
 * largest remaining score, nms.c:74-81) and what mpn_bbox_vote_batched keeps (voted rows carry their NMS scores, nms.c:139).  Only the first
 * min(k, n_c) rows of each class can reach the k-th largest score and a class's survivors are a prefix of it, so the kernel stages
 * n_cls * k keys instead of every kept row.  Same outputs, bit for bit, as mpn_keep_top_k ON SUCH TABLES; on unsorted tables use
 * mpn_keep_top_k.  The test_one forms of the pipeline call this one. */
int mpn_keep_top_k_sorted(const float *d_keep, const int *d_n_keep, int n_cls, int m_stride, int k, float *d_thresh,
                          float *d_out, int max_out, int *d_n_out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Wire formats either side of the path
 * ---------------------------------------------------------------------------------------------- */

/* testCoco/init.lua:65-85: {x1,y1,x2,y2,score,class} rows (mpn_keep_top_k output) -> COCO result rows
 * {image_id, x1-1, y1-1, x2-x1, y2-y1, score, category_id}; d_cat_ids [n_cat] maps class (1-based) to the
 * dataset's category id (NULL: the class index itself).  d_n_dets (device int, may be NULL) bounds max_n. */
int mpn_dets_to_coco_rows(const float *d_dets, const int *d_n_dets, int max_n, float image_id, const float *d_cat_ids,
                          int n_cat, float *d_rows, void *stream);

/* DataSetJSON.lua:157-239 (loadROIDB): proposal rows come as {y1,x1,y2,x2}; emits the {2,1,4,3}-permuted
 * {x1,y1,x2,y2} rows and, in d_keep (may be NULL), 1 for rows whose area (x2-x1)*(y2-y1) > min_area
 * (min_area == 0 keeps everything — filterArea, DataSetJSON.lua:172-186). */
int mpn_proposals_permute_filter(const float *d_in, int n, float min_area, float *d_out, int *d_keep, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Fused per-image pipeline: Tester_FRCNN:testOne -> ImageDetect:detect -> model:forward -> NMS
 * (Tester_FRCNN.lua:54-139, ImageDetect.lua:156-193, models/vgg.lua:23-31)
 * ---------------------------------------------------------------------------------------------- */

typedef struct mpn_frcnn_config {
  int n_conv;              /* number of 3x3 conv layers in the trunk (VGG-16: 13) */
  const int *conv_cout;    /* [n_conv] output channels */
  const int *pool_after;   /* [n_conv] 1 = ceil-mode 2x2 max-pool after this layer's ReLU */
  int pooled_h, pooled_w;  /* ROIPooling bins (VGG: 7,7) */
  float spatial_scale;     /* VGG: 1/16 */
  int fc_dim;              /* 4096 */
  int n_classes;           /* C incl. background (VOC: 21) */
  int max_h, max_w;        /* largest input image (600 x 1000) */
  int max_rois;            /* largest ROI batch (1000) */
  double tf_scale;         /* ImageTransformer: scale, mean[3], std[3] (std[0]==0 -> none), swap[3] */
  double tf_mean[3];
  double tf_std[3];
  int tf_swap[3];         /* output channel j reads image plane tf_swap[j]; a value outside 0..2 is refused at create */
  float bbox_mean[4];      /* BBoxNorm (std[0]==0 -> module absent) */
  float bbox_std[4];
  float nms_thresh;        /* 0.3 */
  float score_thresh;      /* -1.5 (Tester_FRCNN.lua:50) */
  int top_k;               /* 100 (Tester_FRCNN.lua:163) */
  /* accuracy knobs of Tester_FRCNN (all off in the reference's default config): */
  int num_iter;            /* opt.test_num_iterative_loc (1 = off; i = 2..num_iter: SelectBoxes + a head-only pass on the cached
                              trunk features; num_iter * max_rois <= MPN_NMS_MAX_BOXES) */
  int bbox_voting;         /* opt.test_bbox_voting */
  float bbox_vote_thresh;  /* opt.test_bbox_voting_nms_threshold (0.5).  The reference passes an unset field here
                              (Tester_FRCNN.lua:123 vs :29); we use the configured threshold. */
  float bbox_vote_score_pow; /* opt.test_bbox_voting_score_pow (1) */
  /* getImages (ImageDetect.lua:34-43): 0 = feed the image as it is; otherwise rescale so that the short side is
   * scale_target (600), capped so that the long side stays <= scale_max (1000).  max_h / max_w bound the RESCALED image. */
  double scale_target, scale_max;
  int use_rbox_scores;     /* opt.test_use_rbox_scores (Tester_FRCNN.lua:91-97): needs num_iter > 1; the scores of pass i+1 are
                              paired with the boxes of pass i (the first score table and the last box table are dropped), so
                              (num_iter - 1) * N rows reach the NMS */
  int roi_bin_rule;        /* MPN_ROI_BINS_CAFFE (0, default: inn.ROIPooling's CUDA branch) | MPN_ROI_BINS_ADAPTIVE (its CPU branch): the
                              rule of every ROI pooling of the pipeline — mpn_roi_pool_forward_rule.  (added in MPN_VERSION 600, at the END) */
  int fc_arith;            /* MPN_FC_FP32 (0, default): fc6 on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32).  MPN_FC_SPLIT3 (1; mpn_frcnn_create / mpn_mpnet_create): fc6 and fc7
                              on the bf16 pipe with fp32-level results — both operands split exactly into three bf16 planes (h + m + l = the fp32 value),
                              the six plane products of weight >= 2^-16 accumulated in fp32, the three <= 2^-24 ones (the size of an fp32 product's own
                              rounding) dropped.  An AUXILIARY arithmetic: the headline and every parity claim are MPN_FC_FP32.  (MPN_VERSION 600)
                              Edge values, both arithmetics: every output is NaN / +inf / -inf / finite exactly when the float64 sum is (inf x 0
                              and inf - inf give NaN); the ReLU is t < 0 ? 0 : t, so NaN passes through it.  MPN_FC_SPLIT3 specifics: a finite
                              |x| >= 3.3962e38 (where bf16 rounding overflows) keeps h = +-bf16's largest finite value and still splits exactly;
                              a non-finite x is carried in h alone; an fp32 subnormal below bf16's 2^-133 grid is carried to within 2^-134
                              absolutely (the only inexact split), and a weight with 0 < |w| < 2^-134 counts as zero against an infinite x. */
} mpn_frcnn_config;
#define MPN_FC_FP32 0
#define MPN_FC_SPLIT3 1

typedef struct mpn_frcnn mpn_frcnn; /* opaque */

/* Builds the pipeline on the current device: allocates activations/workspace once, re-packs weights
 * into MFMA-fragment order in HBM.  Weight pointers are DEVICE pointers in Torch layout
 * (conv [Cout,Cin,3,3]; linear [out,in]); they are read during this call only.
 * d_conv_w/d_conv_b: arrays (host) of n_conv device pointers. */
int mpn_frcnn_create(const mpn_frcnn_config *cfg, const float *const *d_conv_w, const float *const *d_conv_b,
                     const float *d_fc6_w, const float *d_fc6_b, const float *d_fc7_w, const float *d_fc7_b,
                     const float *d_cls_w, const float *d_cls_b, const float *d_bbox_w, const float *d_bbox_b,
                     mpn_frcnn **out);
/* The same handle with the integral loss's K classifiers (model_utils.lua:275-317, opt.integral on models/vgg.lua): d_cls_w
 * [K*C, F] and d_cls_b [K*C] are the K clones of the classifier stacked in head order, n_integral = K in 1..MPN_MAX_INTEGRAL
 * (the reference's scripts use 6).  The fused head becomes ONE Linear of (K+4)*C rows [cls_0 | .. | cls_{K-1} | bbox]; the scores
 * every form returns (detect, test_one, the pipelined and host-fed forms, iterative localisation, the pyramid, flip augmentation,
 * captured graphs) are the mean over k of softmax(cls_k) — summed in k order, then * (1/K), as nn.Mean —, the boxes are decoded
 * from the one bbox regressor.  n_integral == 1 IS mpn_frcnn_create (which calls this with 1): the same code, the same bits.
 * K > 1 with n_classes > 256 answers MPN_EINVAL (the integral score kernel's limit, as for the tower models); NULL pointers and K
 * out of range answer MPN_EINVAL before any device work.  On a K > 1 handle the proposal-sharded forms (mpn_frcnn_shard_head /
 * _shard_nms / _shard_finish, mpn_frcnn_test_one_sharded) answer MPN_ESTATE: sharding K classifiers is not supported.
 * Training such a handle: mpn_frcnn_train_set_head below. */
#define MPN_MAX_INTEGRAL 8
int mpn_frcnn_create_integral(const mpn_frcnn_config *cfg, const float *const *d_conv_w, const float *const *d_conv_b,
                              const float *d_fc6_w, const float *d_fc6_b, const float *d_fc7_w, const float *d_fc7_b,
                              const float *d_cls_w /*[K*C, F]*/, const float *d_cls_b /*[K*C]*/, const float *d_bbox_w,
                              const float *d_bbox_b, int n_integral, mpn_frcnn **out);
/* K of the handle: mpn_frcnn_create_integral's n_integral, the towers' K for a tower model, 1 for every other handle. */
int mpn_frcnn_n_integral(const mpn_frcnn *p);
void mpn_frcnn_destroy(mpn_frcnn *p);

/* MultiPathNet head (models/multipathnet.lua:64-120): nn.Foveal -> n_towers region towers, each
 * {conv345Combine (model_utils.lua:209-251: ROI pools of conv5 @scale, conv4 @2*scale, conv3 @4*scale,
 * per-map nn.Normalize(2), channel concat, *1000, 1x1 conv mix to conv5's width) -> fc6 -> fc7};
 * the first n_towers-1 ("foveal") towers are concatenated for the K integral classifiers
 * (model_utils.lua:275-317: eval = mean of the K softmaxes), the last ("het") tower feeds the box
 * regressor.  This replaces nn.ModelParallelTable's broadcast/concat (ModelParallelTable.lua:195-242)
 * with zero-copy concatenation on one GPU.  All pointers are device pointers in Torch layout:
 * mix_w[t] [c5, total_feat_t] (the 1x1 conv), fc6_w[t] [fc, c5*PH*PW], fc7_w[t] [fc, fc];
 * d_cls_w [n_integral*C, (n_towers-1)*fc] (the K classifiers stacked), d_bbox_w [4C, fc]. */
typedef struct mpn_mpnet_weights {
  int n_towers;              /* 5 in the reference: regions {0,1,2,3} + het on region 1 */
  int region[8];             /* 0-based Foveal region of each tower (Foveal.lua:36-39 rows) */
  int use_conv4[8], use_conv3[8];
  int tap_conv3, tap_conv4;  /* 0-based conv-layer indices whose pre-pool outputs are "conv3"/"conv4" (VGG-16: 6, 9) */
  int n_integral;            /* K (opt.nDonkeys in the reference, 6 in scripts/train_multipathnet_coco.sh:8) */
  const float *mix_w[8], *mix_b[8], *fc6_w[8], *fc6_b[8], *fc7_w[8], *fc7_b[8];
  int conv345_unnormalized;  /* 0 (default, opt.model_conv345_norm = true): per-map nn.Normalize(2) then MulConstant(1000);
                              * 1: the isNormalized = false branch, MulConstant(1), (1/30), (1/200) on conv5 / conv4 / conv3 and
                              * no x1000 (model_utils.lua:214-223,231-244).  (added in MPN_VERSION 201, at the END of the struct) */
} mpn_mpnet_weights;
int mpn_mpnet_create(const mpn_frcnn_config *cfg, const float *const *d_conv_w, const float *const *d_conv_b,
                     const mpn_mpnet_weights *mw, const float *d_cls_w, const float *d_cls_b, const float *d_bbox_w,
                     const float *d_bbox_b, mpn_frcnn **out);

/* ResNet Fast R-CNN (models/resnet.lua:24-50): net:get(1..7) = conv1 7x7/2, BN, ReLU, max-pool 3x3/2 pad 1,
 * layer1-3 run on the image; inn.ROIPooling(14,14,1/16); net:get(8..10) = layer4 + 7x7 average pool + View run per ROI;
 * classAndBBoxLinear on the pooled vector.  The fb.resnet.torch `.t7` is not in the tree: the caller describes the graph —
 * every convolution in execution order (conv1, then per residual block its convolutions followed by its shortcut
 * convolution if it has one), BatchNorm already folded into w / b (inn.utils.BNtoFixed, resnet.lua:34-36).  A block is
 * relu(conv_n(... relu(conv_1(x)) ...) + shortcut(x)).  Uses cfg->{max_h,max_w,max_rois,n_classes,pooled_h,spatial_scale,
 * tf_*,bbox_*,nms_*,score_thresh,top_k,num_iter,bbox_voting,...}; cfg->n_conv / conv_cout / pool_after / fc_dim are ignored.
 * All pointers are device pointers; fp32. */
typedef struct mpn_resnet_weights {
  int n_convs;
  const float *const *w;       /* [n_convs] -> [cout, cin, k, k] */
  const float *const *b;       /* [n_convs] -> [cout] (may be NULL = no biases) */
  const int *cin, *cout, *ksize, *stride, *pad;   /* [n_convs] */
  int n_blocks;
  const int *block_n_convs;       /* [n_blocks] convolutions on the residual path */
  const int *block_has_shortcut;  /* [n_blocks] 1 = a shortcut convolution follows the block's convolutions in the list */
  int n_trunk_blocks;             /* blocks [0, n_trunk_blocks) = layer1-3 (image trunk); the rest = layer4 (per-ROI head) */
  /* MultiPathNet on a ResNet backbone (BASELINE configs[3]).  The reference tree has NO such model: this is
   * this library's extension, shaped like models/multipathnet.lua:64-120 — nn.Foveal regions over the single stride-16 map, one
   * layer4 copy ("tower") per region, the classification towers' pooled vectors concatenated for n_integral classifier clones
   * (mean of their softmaxes, model_utils.lua:296-315), the LAST tower feeding the box regressor.  n_heads <= 1: plain
   * resnet.lua.  n_heads >= 2: the blocks after the trunk are n_heads equal groups in tower order; d_cls_w is
   * [n_integral*C, (n_heads-1)*out_c], d_bbox_w [4C, out_c]. */
  int n_heads;
  int head_region[8];             /* 0-based Foveal region of each tower */
  int n_integral;
  int bf16;                       /* 1: trunk and per-ROI convolutions in bf16 (bf16 activations and weights, fp32 accumulate; bias, residual,
                                     ReLU in fp32; the cls / bbox head stays fp32) — the dtype SURVEY §8f rank 3 asks for.  0: fp32 */
} mpn_resnet_weights;
int mpn_resnet_create(const mpn_frcnn_config *cfg, const mpn_resnet_weights *rw, const float *d_cls_w, const float *d_cls_b,
                      const float *d_bbox_w, const float *d_bbox_b, mpn_frcnn **out);

/* Branching conv graphs (models/inceptionv3.lua:27-43, BASELINE configs[4]; models/alexnet.lua:14-27, BASELINE configs[0], whose
 * `top` — fc6 / fc7 on the flattened 6x6 ROI-pooled map — is a 6x6 and a 1x1 convolution in the head list): the trunk (net:get(1..25)) and the per-ROI
 * classifier (net:get(26..30)) as two op lists over numbered tensors.  Tensor 0 of the trunk list is the transformed image
 * (3 channels); tensor 0 of the head list is the ROI-pooled map (cfg->pooled_h x pooled_w, channels of `feat_tensor`); the head's
 * `out_tensor` is averaged over its whole map (the graph's final SpatialAveragePooling + View) and feeds classAndBBoxLinear.
 * An op reads ALL channels of `src` and writes `cout` (conv) / src's (pools) channels of `dst` starting at channel
 * `dst_c_off` — an Inception module's DepthConcat is its branches writing side by side into one tensor (offsets and widths
 * must be multiples of 8; of 16 with bf16).  BatchNorm folded into w / b by the caller (utils.BNtoFixed, inceptionv3.lua:23).
 * The `.t7` (Moodstocks' conversion of Google's Inception-v3) is not in the tree: PARITY UNPINNED, structure from the public
 * definition.
 * Convolution edge values: without ReLU (relu = 0, or the channels a fused sibling keeps linear) every output is NaN / +inf / -inf /
 * finite exactly when the float64 sum is (inf x 0 and inf - inf give NaN), except on the fp32 Winograd forms (3x3 / stride 1: the trunk's
 * layers and the per-ROI mosaic), whose transforms spread a non-finite input over its 4x4 input tile.  ReLU(NaN): 0 on bf16 graphs and
 * on the fp32 Winograd forms (as Torch's Threshold), NaN on the other fp32 forms (t < 0 ? 0 : t, like the fully-connected GEMM).  A Winograd
 * layer follows its rule in every launch: the tiles a split-K or tail-split launch finishes in the reduce kernel give 0 as well.
 * The trunk's ceil-mode 2x2 max-pool, fused into a convolution or on its own: the NaNs of a window are ignored, a window holding only
 * NaN gives -inf (v > m from -inf, the CPU oracle's rule) in every kernel that pools: the graph's max-pools and the ROI poolings of both
 * dtypes follow the same rule (the bf16 ROI pooling on the order-preserving int16 image of the map encodes a NaN as -inf; the range-max
 * tables the MultiPathNet towers pool through drop a NaN on either side of every comparison, so they give what the direct kernel gives; a bin
 * that holds nothing above -inf reports arg-max -1, as an empty one does).  An EMPTY ROI bin
 * gives 0.  The sign of a zero maximum is not specified: a window holding both zeros gives the zero met first (row-major) in the kernels that
 * compare floats and +0 in the bf16 ROI pooling on the int16 image and its fused max-pool. */
typedef struct mpn_graph_op {
  int kind;               /* 0 = convolution (+ bias, ReLU if relu), 1 = max-pool (padded cells never win; floor mode unless ceil_mode),
                             2 = average pool, count_include_pad (nn.SpatialAveragePooling's default: always / (kh*kw)),
                             3 = cross-channel LRN, nn.SpatialCrossMapLRN(size = kh, lrn_alpha, lrn_beta, lrn_k) (alexnet.lua's trunk):
                                 out_c = in_c * (lrn_k + lrn_alpha / size * sum_{|c' - c| <= (size-1)/2} in_c'^2) ^ -lrn_beta */
  int src, dst, dst_c_off;
  int cin, cout;          /* conv: weight shape [cout, cin, kh, kw]; pools: cin = channels of src */
  int kh, kw, sh, sw, ph, pw;
  int relu;
  const float *w, *b;     /* conv only, device pointers */
  int src_c_off;          /* the op reads channels [src_c_off, src_c_off + cin) of `src` (a multiple of 8; 0 = from the first): a grouped
                             convolution (alexnet.lua's conv2 / conv4 / conv5, groups = 2) is one op per group */
  int ceil_mode;          /* max-pool: nn.SpatialMaxPooling(...):ceil() / Caffe output size — ceil((H + 2p - k) / s) + 1, minus one when the
                             last window would start beyond the padded input */
  float lrn_alpha, lrn_beta, lrn_k;   /* kind 3 */
} mpn_graph_op;
typedef struct mpn_graph_weights {
  int n_trunk_ops;  const mpn_graph_op *trunk_ops;  int n_trunk_tensors;  const int *trunk_tensor_c;  int feat_tensor;
  int n_head_ops;   const mpn_graph_op *head_ops;   int n_head_tensors;   const int *head_tensor_c;   int out_tensor;
  int bf16;               /* as mpn_resnet_weights.bf16 */
  /* MultiPathNet towers on this backbone (BASELINE configs[4]; this library's extension, see mpn_resnet_weights.n_heads):
   * n_heads >= 2: head_ops holds n_heads * n_head_ops entries, tower-major, every tower the same op structure with its own
   * weights; tower t pools Foveal region head_region[t]; the last tower feeds the box regressor. */
  int n_heads;
  int head_region[8];
  int n_integral;
} mpn_graph_weights;
int mpn_graph_create(const mpn_frcnn_config *cfg, const mpn_graph_weights *gw, const float *d_cls_w, const float *d_cls_b,
                     const float *d_bbox_w, const float *d_bbox_b, mpn_frcnn **out);

/* ImageDetect:detect (ImageDetect.lua:156-193; getImages' rescaling per cfg.scale_target):
 * d_image [3,H,W] fp32 in [0,1]; d_boxes [N,4].  Outputs (all optional, device):
 *   d_scores [N,C] softmax, d_bbox [N,4C] decoded boxes.  clamp = 0 returns them as ImageDetect:detect does (unclamped);
 *   clamp = 1 additionally applies Tester_FRCNN.lua:75-78's clamp to the image, which the reference applies to the FIRST
 *   detect() of testOne only (passes 2..num_iter of iterative localisation stay unclamped, Tester_FRCNN.lua:82-89).
 * d_image == NULL means recompute_features = false (ImageDetect.lua:107-111): the trunk output of the previous
 * call on this handle is reused and only the ROI head runs on the new boxes (iterative localisation,
 * Tester_FRCNN.lua:82-89); H, W must equal the cached image's size. */
int mpn_frcnn_detect(mpn_frcnn *p, const float *d_image, int H, int W, const float *d_boxes, int N, float *d_scores,
                     float *d_bbox, int clamp, void *stream);

/* Tester:testOne + keep_top_k: detect, per-class NMS, global top-k.
 *   d_dets [top_cap,6] {x1,y1,x2,y2,score,class}, *d_n_dets; raw per-class NMS results stay readable
 *   through mpn_frcnn_nms_results until the next call.
 * CONTRACT of *d_n_dets (all test_one forms, as mpn_keep_top_k's *d_n_out): the UNTRUNCATED number of survivors of the
 * top-k rule.  utils.keep_top_k keeps every row tied at the threshold, so it can exceed top_k and even top_cap; only
 * min(*d_n_dets, top_cap) rows of d_dets were written.  A caller must clamp before it reads rows — copy
 * min(n, top_cap) * 6 floats — and may treat n > top_cap as "rows were dropped, enlarge top_cap". */
int mpn_frcnn_test_one(mpn_frcnn *p, const float *d_image, int H, int W, const float *d_boxes, int N, float *d_dets,
                       int top_cap, int *d_n_dets, void *stream);
/* Throughput form for a loop over images (Tester:test, Tester_FRCNN.lua:150-157): same work, but the
 * latency-bound NMS + top-k tail of image i runs on an internal side stream (default priority) and overlaps image
 * i+1's trunk.  d_dets / d_n_dets of call i are ordered on `stream` only after call i+1 (on the same
 * handle) or mpn_frcnn_flush(); alternate two output buffers between consecutive calls.  For the plain Fast R-CNN head
 * (one localisation pass) the class / box GEMM, softmax, decode and select of image i run on that internal stream as well
 * (51 us of kernels that leave most of the GPU idle, now under image i+1's first layers); what they read is kept per
 * buffer set inside the handle — d_image and d_boxes are consumed on `stream` before the call's work there ends, exactly as
 * in the un-pipelined form. */
int mpn_frcnn_test_one_pipelined(mpn_frcnn *p, const float *d_image, int H, int W, const float *d_boxes, int N,
                                 float *d_dets, int top_cap, int *d_n_dets, void *stream);
int mpn_frcnn_flush(mpn_frcnn *p, void *stream);
/* The same throughput form fed from HOST buffers, as the reference's loop is (Tester_FRCNN.lua:64-66 gets a CPU image and
 * CPU boxes; ImageDetect.lua:148-151 copies them to the GPU): the upload of image i (7.2 MB + 16 KB at 600x1000 / 1000 ROIs)
 * runs on the handle's copy stream into one of three handle-owned staging sets and overlaps image i-1's kernels; `stream`
 * waits for it only where the trunk starts.  A staging set is reused once the image that filled it three calls earlier has
 * been consumed: the call waits for that on the HOST (a copy that depends on a compute-queue event leaves the DMA engines),
 * so the host runs at most three images ahead of the device.  h_image / h_boxes should be pinned (hipHostMalloc / hipHostRegister /
 * torch pin_memory) — pageable memory works but serialises the copy; they may be reused as soon as the call returns
 * only if pinned memory is NOT rewritten before the copy ran: alternate two host buffers like the output buffers. */
int mpn_frcnn_test_one_pipelined_host(mpn_frcnn *p, const float *h_image, int H, int W, const float *h_boxes, int N,
                                      float *d_dets, int top_cap, int *d_n_dets, void *stream);
int mpn_frcnn_nms_results(mpn_frcnn *p, const float **d_keep, const int **d_keep_idx, const int **d_n_keep,
                          int *m_stride);
/* ------------------------------------------------------------------------------------------------
 * Multi-GPU: images shard across GPUs, the only exchange is an RCCL all-gather of SCORED BOXES
 * (replaces test_runner.lua:91-104's result hand-back and ModelParallelTable.lua:204-236's feature broadcast)
 * ---------------------------------------------------------------------------------------------- */
typedef struct mpn_comm mpn_comm; /* opaque: one RCCL communicator rank, bound to the device current at creation */
#define MPN_UNIQUE_ID_BYTES 128
/* One process per GPU: rank 0 calls mpn_comm_get_unique_id and hands the 128 bytes to the other ranks out of band
 * (a file, an env var, torch.distributed's store ...); every rank then calls mpn_comm_init_rank (collective).
 * world == 1 with id128 == NULL never loads RCCL (the gather degenerates to the pack kernel); world == 1 with an id
 * creates a real one-rank communicator. */
int mpn_comm_get_unique_id(void *id128);
int mpn_comm_init_rank(const void *id128, int world, int rank, mpn_comm **out);
/* The reference's process model — ONE process, one worker thread per GPU (test_runner.lua:55-66): creates the n_dev
 * communicators at once; worker i uses out[i] with device h_devices[i] (NULL: device i) current. */
int mpn_comm_init_all(int n_dev, const int *h_devices, mpn_comm **out);
int mpn_comm_world(const mpn_comm *c);
int mpn_comm_rank(const mpn_comm *c);
/* What RCCL ITSELF reports for the communicator (ncclCommCount), 0 when there is none (world 1 without an id), -1 when the loaded RCCL
 * has no ncclCommCount symbol (nothing was cross-checked: UNVERIFIED, never the caller's own world size).  Both init entries
 * cross-check ncclCommCount / ncclCommUserRank against the caller's (world, rank) and fail with MPN_ENCCL on a mismatch, and
 * mpn_comm_init_rank waits a bounded time for its peers (MPN_COMM_INIT_TIMEOUT_S, default 120 s) instead of hanging: a multi-GPU
 * run can state — and a bench line can carry — how many ranks RCCL really saw (test_runner.lua:55-66: worker k IS GPU k). */
int mpn_comm_rccl_ranks(const mpn_comm *c);
void mpn_comm_destroy(mpn_comm *c);
/* A rank's record for one image: top_cap rows {x1,y1,x2,y2,score,class} (rows at / beyond the count zeroed) + the count
 * as a float = top_cap*6 + 1 floats (~10 KB for top_cap = 464). */
size_t mpn_det_record_floats(int top_cap);
int mpn_pack_det_record(const float *d_dets, const int *d_n_dets, int top_cap, float *d_rec, void *stream);
/* Packs this rank's (d_dets, *d_n_dets) — mpn_frcnn_test_one's outputs — and all-gathers the records of all ranks into
 * d_out [world, top_cap*6 + 1]; record r belongs to the image rank r processed in this step.  Stream-ordered on
 * `stream`, no host synchronisation; every rank must call it the same number of times. */
int mpn_gather_dets(mpn_comm *c, const float *d_dets, const int *d_n_dets, int top_cap, float *d_out, void *stream);
/* Generic fixed-size all-gather of float records: every rank contributes n_floats from d_send, d_out is [world, n_floats]
 * (rank order).  Stream-ordered, no host synchronisation; without an RCCL communicator (world 1) a device copy.  The calling
 * thread's current device must be the communicator's (MPN_ESTATE otherwise; mpn_gather_dets checks the same). */
int mpn_gather_rows(mpn_comm *c, const float *d_send, size_t n_floats, float *d_out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * COCO box evaluation — testCoco/coco.lua:24-37 `Coco:evaluate` (pycocotools COCOeval, iouType 'bbox') on the device
 * ---------------------------------------------------------------------------------------------- */
typedef struct mpn_coco_eval mpn_coco_eval; /* opaque: one GT set + parameters, bound to one device */
#define MPN_COCO_MAX_DETS 1024
/* The GT arrays are in annotation-file order: h_gt_bbox [n_gt,4] {x,y,w,h} and h_gt_area as in the JSON, iscrowd / image id /
 * category id / annotation id as int64.  h_img_ids [n_img]: the GT set's image ids (COCO.getImgIds()), strictly increasing; rows
 * naming any other image are refused by _run (loadRes's assert), GTs of other images are never read.  h_eval_img_ids == NULL
 * evaluates the images that have at least one row (coco.lua:28-30); otherwise params.imgIds = h_eval_img_ids [n_eval].
 * h_cat_ids [n_cat] strictly increasing (params.catIds).  h_iou_thrs [n_iou], h_rec_thrs [n_rec], h_area_rng [n_area,2] (both ends
 * closed), h_max_dets [n_max_dets] (each 1..MPN_COCO_MAX_DETS; the images are evaluated with the last one) are pycocotools' Params,
 * passed as they are: n_iou * n_area <= 64, n_area <= 8.  Arguments are validated before the device is touched; device < 0 = the
 * current device.  The handle allocates its GT tables here and its per-row buffers on the first _run of a larger n. */
int mpn_coco_eval_create(int device, const double *h_gt_bbox, const double *h_gt_area, const int64_t *h_gt_iscrowd,
                         const int64_t *h_gt_image_id, const int64_t *h_gt_category_id, const int64_t *h_gt_id, int n_gt,
                         const int64_t *h_img_ids, int n_img, const int64_t *h_eval_img_ids, int n_eval, const int64_t *h_cat_ids,
                         int n_cat, const double *h_iou_thrs, int n_iou, const double *h_rec_thrs, int n_rec, const double *h_area_rng,
                         int n_area, const int *h_max_dets, int n_max_dets, mpn_coco_eval **out);
/* evaluate + accumulate of d_rows [n,7] fp32 {image, x, y, w, h, score, category} (testCoco/init.lua:65-85's `boxt`) into
 * d_precision / d_scores [T,R,K,A,M] and d_recall [T,K,A,M], float64, -1 where pycocotools leaves -1.
 * Deterministic.  Unlike the module-level calls it synchronises `stream` once at the end: a row naming an image outside h_img_ids,
 * or holding a NaN / inf, returns MPN_EINVAL (the outputs are then unspecified).  Drive one handle from one thread at a time, with
 * its device current (MPN_ESTATE otherwise). */
int mpn_coco_eval_run(mpn_coco_eval *h, const float *d_rows, int n, double *d_precision, double *d_recall, double *d_scores,
                      void *stream);
void mpn_coco_eval_destroy(mpn_coco_eval *h);

/* ------------------------------------------------------------------------------------------------
 * Proposal (ROI) sharding of ONE image across the GPUs of a node — the latency mode (north_star "images+proposals
 * shard across the 8 GPUs").  Replaces ModelParallelTable.lua:195-242 (broadcast the input to every tower GPU, run, copy back,
 * concatenate) for a single image: every rank holds the full model and is handed the SAME image and the SAME proposal table;
 * it runs the trunk, the ROI head on its contiguous slice of the proposals (mpn_shard_range(N, world, rank)), the per-class NMS
 * on its contiguous slice of the foreground classes (mpn_shard_range(C-1, world, rank)), and two all-gathers of scored boxes
 * connect the three steps.  Rows and classes are independent, so d_dets / d_n_dets and mpn_frcnn_nms_results equal the
 * unsharded mpn_frcnn_test_one's bit for bit on every rank; iterative localisation and box voting are supported (each rank
 * refines its own rows).  The partition contract is test_runner.lua:91-104's (every worker the same code, a disjoint share).
 *   mpn_frcnn_shard_head   trunk + head on this rank's proposals -> d_rows_rec [mpn_frcnn_shard_rows_floats]
 *   (exchange)             d_rows_all [world, rows_floats] = all ranks' records in rank order (mpn_gather_rows or any transport)
 *   mpn_frcnn_shard_nms    joined tables of the whole image (kept on the handle: what detect() returns), select, NMS (+ vote)
 *                          of this rank's classes -> d_class_rec [mpn_frcnn_shard_class_floats]
 *   (exchange)             d_class_all [world, class_floats]
 *   mpn_frcnn_shard_finish every class's kept table on the handle (mpn_frcnn_nms_results) + keep_top_k -> d_dets, *d_n_dets
 * mpn_frcnn_test_one_sharded chains the five steps over an mpn_comm on `stream` (no host synchronisation in steady state).
 * The same image size / N / world must be passed to all steps; a rank that owns no proposals (world > N) writes a zero record. */
int mpn_shard_range(int n, int world, int rank, int *lo, int *hi); /* balanced contiguous: the first n % world ranks own one more */
size_t mpn_frcnn_shard_rows_floats(const mpn_frcnn *p, int N, int world);
size_t mpn_frcnn_shard_class_floats(const mpn_frcnn *p, int N, int world);
int mpn_frcnn_shard_head(mpn_frcnn *p, const float *d_image, int H, int W, const float *d_boxes, int N, int rank, int world,
                         float *d_rows_rec, void *stream);
int mpn_frcnn_shard_nms(mpn_frcnn *p, const float *d_rows_all, int N, int rank, int world, float *d_class_rec, void *stream);
int mpn_frcnn_shard_finish(mpn_frcnn *p, const float *d_class_all, int N, int world, float *d_dets, int top_cap, int *d_n_dets,
                           void *stream);
int mpn_frcnn_test_one_sharded(mpn_frcnn *p, mpn_comm *comm, const float *d_image, int H, int W, const float *d_boxes, int N,
                               float *d_dets, int top_cap, int *d_n_dets, void *stream);

/* Multi-scale testing (Fast R-CNN's image pyramid; getImages + project_im_rois with a scale TABLE, ImageDetect.lua:22-73; DESIGN.md
 * section 11).  h_targets [n_scales] are getImages' targets t_l; cfg.scale_max stays the cap.
 *   n_scales == 0 restores the creation-time cfg.scale_target (single scale); n_scales == 1 sets scale_target = t_0 (single scale,
 *   today's path bit for bit); 2 <= n_scales <= MPN_MAX_SCALES sets the pyramid.  Targets must be finite and > 0.  Arguments are
 *   checked before the device is touched; the call synchronises the device, drops every captured launch graph of the handle and
 *   the cached trunk output (the next detect must pass an image), and allocates the per-level map slots on first use.
 * With a pyramid, for an image [3,H0,W0]: s_l = mpn_pick_scale(H0, W0, t_l, scale_max), level size (H_l, W_l) = ((int)(H0*s_l),
 * (int)(W0*s_l)), each level resampled and transformed as the single-scale image is and placed top-left in a zero canvas
 * (max H_l) x (max W_l) (0 in the transformed domain); the whole trunk runs on every canvas; every ROI is levelled and projected
 * as mpn_project_im_rois_levels does and pools from its level's map; heads, softmax, decode on the ORIGINAL boxes, clamp to the
 * ORIGINAL image, NMS, voting and top-k are unchanged.  Levels with a scale equal to an earlier level's are computed once (no ROI
 * can pick them).  The canvas must fit max_h x max_w (MPN_EINVAL otherwise).  Supported by mpn_frcnn_detect (cached features
 * included) and mpn_frcnn_test_one (iterative localisation re-levels the refined boxes on the cached maps); the pipelined,
 * host-fed and sharded forms return MPN_EINVAL while a pyramid is set.  Only mpn_frcnn_create handles take a pyramid:
 * mpn_mpnet_create / mpn_resnet_create / mpn_graph_create handles return MPN_EINVAL for n_scales > 1.
 * Debug tensors (mpn_frcnn_debug_tensor) with a pyramid: "conv5.<l>" (level l's final map, NCHW at the canvas geometry) and
 * "rois" ([N,5], the projected table of the last head pass; also kept without a pyramid). */
int mpn_frcnn_set_scales(mpn_frcnn *p, int n_scales, const double *h_targets);

/* Horizontal-flip test-time augmentation (opt.test_augment, run_test.lua:39 — declared in the reference, read by nothing there;
 * completed the standard way).  With enable != 0, for an image im [3,H0,W0] and boxes b [N,4], all in fp32,
 * every operation rounded on its own:
 *   im_f = mpn_image_hflip(im) (the ORIGINAL image, before getImages and the transformer);  b_f = mpn_flip_boxes(b, W0);
 *   (sA, bA) = detect(im, b), (sB, bB) = detect(im_f, b_f): ImageDetect:detect as it is without augmentation, unclamped, scores
 *   after the softmax (after the integral mean for noSoftMax models), bB decoded against b_f in the mirrored frame;
 *   scores = (sA + sB) * 0.5f;  bbox[:, 4c:4c+4] = (bA_c + flipBoxes(bB_c, W0)) * 0.5f for every class c;
 *   then the clamp to [1,W0] x [1,H0] where the caller asked for it (mpn_frcnn_detect's clamp, the first pass of test_one).
 * Select, NMS, voting and top-k see the merged tables only.  Iterative localisation: pass i+1 takes SelectBoxes of the merged
 * tables of pass i and runs both halves on cached trunk maps — the upright map with the new boxes, the mirrored map with their
 * flip; use_rbox_scores pairs the merged tables.  enable == 0: every output of every entry point is what it was before the call.
 * The call synchronises the device, drops every captured launch graph of the handle and the cached trunk output (the next detect
 * must pass an image) and allocates the second half's buffers on first use; any N <= max_rois keeps working.
 * mpn_frcnn_create handles (plain Fast R-CNN heads) keep BOTH trunk maps cached: mpn_frcnn_detect with cached features and every
 * num_iter work.  mpn_mpnet_create / mpn_resnet_create / mpn_graph_create handles run the two halves as two whole passes and keep
 * one map: enabling returns MPN_EINVAL when the handle was created with num_iter > 1, and a cached-features detect returns
 * MPN_EINVAL while augmentation is on.  The pipelined, host-fed and sharded forms return MPN_EINVAL while augmentation is on.
 * Augmentation and an image pyramid (mpn_frcnn_set_scales with more than one target) exclude each other: the setter called second
 * returns MPN_EINVAL.  A refused call changes nothing. */
int mpn_frcnn_set_augment(mpn_frcnn *p, int enable);

/* ------------------------------------------------------------------------------------------------
 * Fine-tuning the Fast R-CNN head on the device, trunk frozen (train.lua:154-158, BatchProviderROI.lua:125-131,
 * BBoxRegressionCriterion.lua, engines/Optim.lua)
 * ------------------------------------------------------------------------------------------------
 * Only a plain VGG Fast R-CNN handle (mpn_frcnn_create, fc_arith == MPN_FC_FP32) trains: fc6, fc7 and the fused cls + bbox head.
 * MultiPathNet, ResNet and op-list handles, MPN_FC_SPLIT3 handles, a handle with an image pyramid or augmentation on, and a handle
 * whose pipelined tail is still pending (until mpn_frcnn_flush) answer MPN_ESTATE with a message naming what refused.
 * After mpn_frcnn_train_begin there is NO dropout (the reference's opt.train_remove_dropouts = true); mpn_frcnn_train_set_dropout
 * switches on the reference's default, the two nn.Dropout(0.5) of models/vgg.lua:21 (below).  Either way a step is deterministic — the
 * same calls on the same inputs, seed and step counter give the same bits (fixed summation orders, no atomics, a counter-based mask).
 *
 *   mpn_frcnn_train_begin  allocates one zeroed momentum buffer per trained tensor, in the packed layout of its weight (fc6's, as
 *                          large as fc6's weights, only at depth MPN_TRAIN_FC6), and the gradient scratch.  A second begin without an
 *                          end: MPN_ESTATE.
 *   mpn_frcnn_train_add    appends one image's n rows to the pending minibatch (total rows <= max_rois, MPN_EINVAL beyond): getImages'
 *                          rescale and the frozen trunk exactly as mpn_frcnn_detect runs them, the ROI projection, the ROI pooling of
 *                          these rows into the minibatch's fc6 operand behind the rows already pending (a buffer of its own: a detect between two
 *                          training calls disturbs nothing); d_rois / d_gt / d_labels are copied.  Boxes are
 *                          in the ORIGINAL image's coordinates, as detect takes them; d_gt[i] is the ground-truth box row i regresses to
 *                          (read only where d_labels[i] > 0).  Flip on the caller's side with mpn_image_hflip / mpn_flip_boxes.  The
 *                          handle's cached trunk features are invalid afterwards: a detect with d_image == NULL returns MPN_ESTATE.
 *   mpn_frcnn_train_step   head forward, loss, backward and SGD update on the B pending rows; clears the batch (MPN_ESTATE with none).
 *                          z = class logits [B,C], t^ = raw box outputs [B,4C] (nn.BBoxNorm is the identity in training), y = labels:
 *                            t_i = (utils.convertTo(roi_i, gt_i) - bbox_mean) / bbox_std for y_i > 0 (bbox_std[0] == 0: not normalised)
 *                            d_loss[0] = (1/B) sum_i -log softmax(z_i)[y_i]                      (log-sum-exp)
 *                            d_loss[1] = (bbox_weight/B) sum_{i: y_i > 0} sum_{j<4} smoothL1(t^_{i,4 y_i + j} - t_{i,j})   (B counts ALL rows)
 *                          backward through heads -> fc7 -> fc6 as far as `depth` says, nothing below the pooled features;
 *                          optim.sgd, dampening 0, no Nesterov: g += weight_decay * w (weights only, biases never decay), v = momentum * v + g,
 *                          w -= lr * v.  The packed weights are updated IN PLACE, where detect's kernels and captured graphs read them:
 *                          a detect after a step uses the new weights, with no re-pack and no re-capture.  d_loss may be NULL.
 *   mpn_frcnn_train_end    frees the momentum buffers and the scratch; the weights stay as trained.
 *   mpn_frcnn_get_head_weights  the current weights back in Torch layout ([out, in]; fc6's `in` index as at creation; cls and bbox split out
 *                          of the fused head); any pointer may be NULL; with or without a train_begin; any mpn_frcnn_create handle.  The exact
 *                          inverse of creation: unpack -> create -> unpack is bit-identical.
 * Debug tensor "train_pooled": fc6's operand of the last step, [B, C, PH, PW] (valid until the next mpn_frcnn_train_add).
 *
 * Below the pooled features: depth MPN_TRAIN_CONV(k), k = 1..K, also trains the last k conv layers of the trunk.  K = the number of conv
 * layers behind the trunk's last pool_after layer (VGG-16: K = 3; k = 1 trains conv5_3, k = 2 adds conv5_2, k = 3 adds conv5_1 — the
 * reference, models/vgg.lua:19, trains conv3_1 and up); k > K answers MPN_EINVAL naming K: a pooling layer is in the way.  With B
 * pending rows of I <= MPN_TRAIN_MAX_IMAGES images (one more mpn_frcnn_train_add: MPN_EINVAL), g6 the gradient at fc6's output:
 *   dx6 = (g6 W6) .* [x6 > 0]      the mask is the last conv layer's ReLU mask (pooled values are post-ReLU map values); it also
 *                                  kills every bin whose argmax sits on a zero cell and every empty bin
 *   per image, in train_add order: dY = mpn_roi_pool_backward's ordered sum over that image's rows into a zero-haloed map; then, last
 *   trained layer to first, with X the layer's saved input map and G the (masked) gradient at its output:
 *     db[co] += sum_pixels G[co]                                    (32 interleaved pixel-ascending sums, then a fixed tree)
 *     dW[co,ci,ky,kx] += sum_{y,x} G[co,y,x] X[ci,y+ky-1,x+kx-1]     (fp32 MFMA over row-major pixel pairs in segments of 512 pixels,
 *                                                                   the segments added in order: fixed by the layer and map size)
 *     dX = conv3x3(G, W rotated by 180 degrees, cin / cout swapped) .* [X > 0]   when a trained layer lies below (the forward's kernels)
 *   optim.sgd exactly as for the head; every input gradient is computed before any weight is updated.
 * The master copy of a trained conv layer is its direct-kernel pack, updated in place; the Winograd pack (and the K = 36 pack of a
 * first layer) are rebuilt in place from it with the packers creation uses, so after a step every form is bit-identical to what
 * creation would build from mpn_frcnn_get_trunk_weights' output, and detect and captured graphs read the same addresses.
 * mpn_frcnn_train_add at these depths also keeps the rows' argmax and copies the block's input map and the trained layers' outputs
 * into per-image slots; mpn_frcnn_train_begin allocates all of it, all or nothing, only at these depths.  VGG-16 at 600 x 1000 with
 * max_rois 1000: 8 images x 4 maps x 6.8 MB = 218 MB, argmax 100 MB, dx6 103 MB, two gradient maps 14 MB, and per trained layer
 * (2.4 M weights) momentum + gradient + the input gradient's two packs, 110 MB for the three, 47 MB of partial sums, 19 MB of
 * Torch-layout scratch: 0.6 GB in all.
 * Through the pooling layers: depth MPN_TRAIN_TRUNK(k), k = 1..min(n_conv - 1, MPN_TRAIN_MAX_TRUNK), trains the ROI head and the last
 * k conv layers counted straight through the pool_after layers (VGG-16, k = 9: conv3_1 and up, the reference's models/vgg.lua:19).  The
 * first conv layer is never trained (its input is the image); a larger k answers MPN_EINVAL naming the limit.  For k <= K it IS
 * MPN_TRAIN_CONV(k): the same code, the same bits.  Beyond K every map has its own size (halved, rounding up, at each pool); per image
 * mpn_frcnn_train_add keeps the first trained layer's input map, every trained layer's post-ReLU output (where the layer is pooled:
 * the map BEFORE the pool) and the pooled map wherever it is the next trained layer's input.  The chain above runs with each layer's
 * own size, and at a pooled layer the gradient arriving at its pooled output first goes through mpn_maxpool2x2_ceil_backward's rule
 * in its relu_mask form (X = the saved pre-pool map) into a zero-haloed map of the larger size — one pass instead of the [X > 0]
 * mask; the input gradient handed to a pooled layer is therefore not masked on its own.  Everything else — the summation orders,
 * every gradient before any update, optim.sgd, the re-pack of the derived forms — is as above.  MPN_TRAIN_MAX_IMAGES applies.
 * Still not trained: the first conv layer, ResNet / op-list handles (a MultiPathNet handle's towers: mpn_mpnet_train_* below).
 * Debug tensors after such a step, until the next mpn_frcnn_train_add: "train_act.<i>.<j>" (image i; j = 0 the block's input map,
 * j = 1..k the trained layers' outputs — before the pool where the layer is pooled; [C,h,w], each map its own h x w) and "train_dx6"
 * ([B, C, PH, PW]).
 *   mpn_frcnn_get_trunk_weights  conv layer `layer`'s current weights [Cout,Cin,3,3] and bias [Cout] in Torch layout (either may be
 *                          NULL); any mpn_frcnn_create handle, with or without training.  The exact inverse of creation.
 *
 * Dropout and resumable runs.  Between mpn_frcnn_train_begin and mpn_frcnn_train_end:
 *   mpn_frcnn_train_set_dropout  nn.Dropout(rate) (v2) in place behind fc6 + ReLU and behind fc7 + ReLU from the next mpn_frcnn_train_step
 *                          on, at EVERY depth (at MPN_TRAIN_HEADS fc6 and fc7 are frozen, but the model is in training mode: the heads see
 *                          the dropped y7).  rate finite in [0, 1), MPN_EINVAL otherwise; 0 switches it off (no kernel is launched, every
 *                          bit is what it is without the call); without a train_begin MPN_ESTATE.  mpn_frcnn_train_begin starts at rate 0.
 *                          No mask is stored; the mask of an element is a function of five integers.  Philox4x32-10 with
 *                            key     = (seed & 0xffffffff, seed >> 32)   (seed taken as 64 bits)
 *                            counter = (row, col >> 2, layer, step & 0xffffffff)
 *                          gives four words; word col & 3 is the element's.  row: the row's index in the pending minibatch (train_add order
 *                          across images); col: the layer's output column; layer: 0 behind fc6, 1 behind fc7; step: the handle's step
 *                          counter — 0 at train_begin, incremented by every mpn_frcnn_train_step that reaches the forward pass, whatever
 *                          the rate (also when a launch then fails); a step's masks use the value before the increment.  With
 *                          T = floor(rate * 2^32) (in double, rate being the float passed; 0.5 -> 0x80000000) the element is KEPT iff
 *                          word >= T.  Kept: fl(x * s), s = 1.0f / (1.0f - rate) in fp32 (rate 0.5: exactly x 2); dropped: +0.0f.
 *                          Backward: the saved activations are the dropped ones, so [x > 0] is keep mask x ReLU mask and the two input
 *                          gradients that cross a dropout (head -> y7, fc7 -> y6) are scaled by s; the weight gradients contract against
 *                          the dropped activations as they are.  Inference (detect, test_one) never sees dropout.
 *   mpn_frcnn_train_get_state  the momentum buffers in Torch layout — the shapes of mpn_frcnn_get_head_weights, cls and bbox split out of
 *                          the fused head — and the step counter (*h_step, a HOST pointer; may be NULL).  A tensor the current depth
 *                          trains may be NULL (not wanted); one it does NOT train has no momentum and MUST be NULL: MPN_EINVAL naming it.
 *   mpn_frcnn_train_set_state  the inverse: packs the momentum as creation packs the weights (pad lanes +0.0; get -> set -> get is exact)
 *                          and sets the step counter (>= 0).  EVERY tensor the depth trains must be given, every other one NULL:
 *                          MPN_EINVAL naming the tensor.  With rows pending (a train_add without its step): MPN_ESTATE.
 *   mpn_frcnn_train_get_trunk_state / _set_trunk_state  the same for one TRAINED conv layer ([Cout,Cin,3,3], [Cout]; the shapes of
 *                          mpn_frcnn_get_trunk_weights); a layer the depth does not train: MPN_EINVAL naming the trained range.  get: either
 *                          pointer may be NULL; set: both are needed, and rows pending answer MPN_ESTATE.
 * The weights (mpn_frcnn_get_head_weights / _get_trunk_weights), this state, the rate and the seed are everything a run continues
 * from: a new handle created from the weights, train_begin, set_dropout, set_state gives the bits of the uninterrupted run (the
 * reference's model_<epoch>.t7 + optimState_<epoch>.t7, train.lua:188-198).
 * Debug tensors "train_y6" / "train_y7": fc6's / fc7's output of the last step as the next layer read it (behind the dropout),
 * [B, fc_dim] row-major, valid until the next mpn_frcnn_train_step.
 *
 * The integral loss (model_utils.lua:275-317, train.lua:288-294).  A K > 1 handle of
 * mpn_frcnn_create_integral trains ONE of its K classifiers per minibatch:
 *   mpn_frcnn_train_set_head  chooses the classifier k in [0, K) whose logits the loss of the NEXT mpn_frcnn_train_step reads — the
 *                          reference's integral_selector.index, which it sets from the donkey index; the caller's schedule decides it.
 *                          mpn_frcnn_train_begin starts at 0.  k outside [0, K): MPN_EINVAL naming K; without a train_begin: MPN_ESTATE.
 *                          It may be called with rows pending (the head is read at the step) and is NOT part of the optimiser state
 *                          (get_state / set_state do not carry it).  A K == 1 handle takes k = 0 only.
 *   mpn_frcnn_train_step   on such a handle: the cross-entropy and its gradient read and write columns [k*C, (k+1)*C) of the fused
 *                          head's row, the box columns are K*C + 4 y + j, and every other classifier's gradient columns are exactly
 *                          +0.0.  The K - 1 unselected classifiers ARE stepped with that zero gradient, as engines/Optim.lua steps every
 *                          module on every call: weight decay and momentum act on them; with momentum 0 and weight decay 0 their bits
 *                          do not change.
 *   mpn_frcnn_get_head_weights, mpn_frcnn_train_get_state / _set_state  on a K > 1 handle d_cls_w / d_cls_v are [K*C, F] and
 *                          d_cls_b / d_cls_vb [K*C], the K classifiers stacked in head order as creation takes them.
 * Debug tensor "cls_k" on a K > 1 plain handle: the K classifiers' logits of the last detect, [N, K*C]; "cls" there answers MPN_EINVAL
 * naming "cls_k". */
#define MPN_TRAIN_HEADS 0   /* cls + bbox linear only          */
#define MPN_TRAIN_FC7   1   /* + fc7                           */
#define MPN_TRAIN_FC6   2   /* + fc6 (the whole ROI head)      */
#define MPN_TRAIN_MAX_IMAGES 8
#define MPN_TRAIN_CONV(k) (MPN_TRAIN_FC6 + (k))   /* + the last k conv layers, k = 1..K (see above) */
enum { MPN_TRAIN_MAX_CONV = 7 };   /* K is capped here: a trunk with more conv layers behind its last pooling layer trains the last 7 */
#define MPN_TRAIN_TRUNK(k) (32 + (k))    /* the ROI head + the last k conv layers of the trunk, pooling layers crossed */
enum { MPN_TRAIN_MAX_TRUNK = 12 };
int mpn_frcnn_train_begin(mpn_frcnn *p, int depth, float momentum, float weight_decay, float bbox_weight);
int mpn_frcnn_train_add(mpn_frcnn *p, const float *d_image, int H, int W, const float *d_rois /*[n,4]*/,
                        const float *d_gt /*[n,4]*/, const int *d_labels /*[n], 0 = background*/, int n, void *stream);
int mpn_frcnn_train_step(mpn_frcnn *p, float lr, float *d_loss /*[2]: cls, bbox*/, void *stream);
int mpn_frcnn_train_end(mpn_frcnn *p);
int mpn_frcnn_train_set_dropout(mpn_frcnn *p, float rate, long seed);
int mpn_frcnn_train_set_head(mpn_frcnn *p, int k);
int mpn_frcnn_train_get_state(mpn_frcnn *p, float *d_fc6_v, float *d_fc6_vb, float *d_fc7_v, float *d_fc7_vb, float *d_cls_v, float *d_cls_vb,
                              float *d_bbox_v, float *d_bbox_vb, long *h_step, void *stream);
int mpn_frcnn_train_set_state(mpn_frcnn *p, const float *d_fc6_v, const float *d_fc6_vb, const float *d_fc7_v, const float *d_fc7_vb,
                              const float *d_cls_v, const float *d_cls_vb, const float *d_bbox_v, const float *d_bbox_vb, long step, void *stream);
int mpn_frcnn_train_get_trunk_state(mpn_frcnn *p, int layer, float *d_v /*[Cout,Cin,3,3]*/, float *d_vb /*[Cout]*/, void *stream);
int mpn_frcnn_train_set_trunk_state(mpn_frcnn *p, int layer, const float *d_v, const float *d_vb, void *stream);
int mpn_frcnn_get_head_weights(mpn_frcnn *p, float *d_fc6_w, float *d_fc6_b, float *d_fc7_w, float *d_fc7_b,
                               float *d_cls_w, float *d_cls_b, float *d_bbox_w, float *d_bbox_b, void *stream);
int mpn_frcnn_get_trunk_weights(mpn_frcnn *p, int layer, float *d_w /*[Cout,Cin,3,3]*/, float *d_b /*[Cout]*/, void *stream);

/* Training the towers of a MultiPathNet handle on the device, trunk frozen: models/multipathnet.lua phase 1 —
 * the whole trunk inside nn.NoBackprop, everything trainable behind the ROI pooling.  Trained: per tower the 1x1 conv_mix, fc6 and fc7,
 * the K classifiers on the Foveal towers' concat and the box regressor on the het tower.  Only an mpn_mpnet_create handle with
 * fc_arith == MPN_FC_FP32; every other handle kind, MPN_FC_SPLIT3, an image pyramid, augmentation switched on, a pending pipelined
 * tail and calls out of order answer MPN_ESTATE with a message naming the cause, and leave the handle usable.  (mpn_frcnn_train_*
 * above keeps refusing MultiPathNet handles: the two families do not mix.)  The protocol is mpn_frcnn_train_*'s:
 *   mpn_mpnet_train_begin  allocates momentum, the step's activations and gradients (its own buffers: a detect between two training
 *                          calls disturbs nothing); no dropout, classifier 0 selected.
 *   mpn_mpnet_train_add    one image's n rows behind the pending ones (total <= max_rois): the frozen trunk as detect runs it, then per
 *                          tower t the operand x_t[(bin, roi), Kcat_t] = the ROI max-pools of conv5 [+ conv4] [+ conv3] at scales s, 2s, 4s
 *                          over Foveal region r_t, each map's slab nn.Normalize(2)-ed per ROI, x 1000 (conv345_unnormalized:
 *                          MulConstant(1, 1/30, 1/200) and no x 1000).  Cached features of the handle are invalidated.
 *   mpn_mpnet_train_step   forward m_t = x_t Wmix^T + bmix (NO ReLU), y6_t = drop(relu(fc6(m_t))), y7_t = drop(relu(fc7(y6_t))) = slice t of
 *                          cat; z = cat[:, 0:(T-1)F] Wcls^T + bcls [B, K*C], t^ = cat[:, (T-1)F:TF] Wbbox^T + bbbox [B, 4C]; loss and its
 *                          gradient exactly mpn_frcnn_train_step's (classifier k's columns of z, smooth-L1 on t^, 1/B and bbox_weight/B);
 *                          every input gradient is taken before the layer it passes through is updated; optim.sgd in place on the packed
 *                          weights detect and captured graphs read (weight decay on weights only, momentum, dampening 0).  The K - 1
 *                          classifiers not selected get an exactly zero gradient and are still stepped.  d_loss [2] may be NULL.
 *                          Deterministic: fixed summation orders that depend on the shapes and B alone, no atomics.
 *   mpn_mpnet_train_end    frees the state; the weights stay as trained.
 *   mpn_mpnet_train_set_dropout  nn.Dropout(rate) behind fc6 + ReLU and fc7 + ReLU of every tower: mpn_frcnn_train_set_dropout's mask
 *                          with layer = 2 t + i (i = 0 behind fc6, 1 behind fc7), so two towers never share a mask; rate 0 launches nothing.
 *   mpn_mpnet_train_set_head  the classifier k in [0, K) the next step's loss reads.
 *   mpn_mpnet_get_tower_weights / _get_head_weights  the weights in Torch layout, the shapes mpn_mpnet_create takes (any pointer may be
 *                          NULL); with or without a train_begin: the exact inverse of creation.
 * Debug tensors of the last step (mpn_frcnn_debug_tensor), row-major: "tower_train_x.<t>" [rows, Kcat_t, PH, PW], "tower_train_y6.<t>"
 * [rows, fc_dim], "tower_train_cat" [rows, T * fc_dim], "tower_train_cls" [rows, K*C], "tower_train_bbox" [rows, 4C], "tower_train_g_cls"
 * [rows, K*C] (the gradient at z).
 *
 * The optimiser state of a tower run, under mpn_frcnn_train_get_state / _set_state's rules:
 *   mpn_mpnet_train_get_state  tower t's momentum in Torch layout — the shapes of mpn_mpnet_get_tower_weights: mix [c5, Kcat_t], fc6
 *                          [F, c5 * PH * PW], fc7 [F, F], each with its bias.  Any pointer may be NULL (not wanted).
 *   mpn_mpnet_train_set_state  the inverse: packs the momentum as creation packs the weights (pad lanes +0.0; get -> set -> get is exact).
 *                          All six tensors are required: a NULL one answers MPN_EINVAL naming it.
 *   mpn_mpnet_train_get_head_state / _set_head_state  the same for the K classifiers [K*C, (T-1) F] and the box regressor [4C, F] — the
 *                          shapes of mpn_mpnet_get_head_weights — and the step counter the dropout masks read (*h_step: a HOST pointer, may be
 *                          NULL; step >= 0, else MPN_EINVAL).  set: all four tensors are required.
 *                          tower outside [0, T): MPN_EINVAL naming T.  Without an mpn_mpnet_train_begin: MPN_ESTATE.  A set with rows pending
 *                          (a train_add without its step): MPN_ESTATE.  Every other handle kind: MPN_ESTATE with mpn_mpnet_train_begin's
 *                          message.  A refused call changes nothing.
 * The weights (mpn_mpnet_get_tower_weights / _get_head_weights), this state, the dropout rate and the seed are everything a tower run
 * continues from: a new handle created from the weights, train_begin, set_dropout, the set_state calls give the bits of the
 * uninterrupted run.
 *
 * The learning-rate drop on the momentum (train.lua:321-335: `dfdx:mul(state.decay)` beside `learningRate * decay`), both kinds:
 *   mpn_frcnn_train_scale_momentum / mpn_mpnet_train_scale_momentum  v <- fl(v * factor) in fp32, one rounding per element, in place on
 *                          EVERY momentum buffer the state holds — plain handle: fc6, fc7 and the head as far as the depth trains them, and
 *                          every trained conv layer; tower handle: every tower's mix / fc6 / fc7 and both heads; weights and biases.
 *                          factor must be finite and >= 0 (MPN_EINVAL otherwise): the pad lanes of the packed buffers stay +0.0.
 *                          factor == 1.0f launches nothing; 0.0f is the reference's reset on a phase switch (train.lua:248-259).  With rows
 *                          pending: MPN_ESTATE (the reference scales between epochs).  One streaming launch per buffer, each byte read
 *                          and written once.  The exported state afterwards is np.float32(v) * np.float32(factor) bit for bit.
 *
 * Phase 2, first step: the conv block above the last pooling layer trained together with the towers (DESIGN.md section 13.15;
 * models/model_utils.lua:184-207 setPhase2 restricted to conv5_1 .. conv5_3 of VGG-16).
 *   mpn_mpnet_train_begin_conv  mpn_mpnet_train_begin that also trains the trunk's last conv_layers = k conv layers, k in 0..K, K = the conv
 *                          layers behind the trunk's last pool_after layer capped at MPN_TRAIN_MAX_CONV, as for MPN_TRAIN_CONV.  k = 0 IS
 *                          mpn_mpnet_train_begin: the same state, the same launches, the same bits.  k < 0 or k > K: MPN_EINVAL naming K;
 *                          every other refusal is mpn_mpnet_train_begin's; the allocation is all or nothing.  With k > 0 at most
 *                          MPN_TRAIN_MAX_IMAGES images may be pending: one more mpn_mpnet_train_add / _add_sampled answers MPN_EINVAL and
 *                          changes nothing.
 *   mpn_mpnet_get_trunk_weights  conv layer `layer`'s weights [Cout,Cin,3,3] and bias [Cout] in Torch layout (either may be NULL), with or
 *                          without training: the exact inverse of creation (mpn_frcnn_get_trunk_weights keeps refusing these handles).
 *   mpn_mpnet_train_get_trunk_state / _set_trunk_state  a TRAINED conv layer's momentum in those shapes, under the rules of
 *                          mpn_frcnn_train_get_trunk_state / _set_trunk_state: get: either pointer may be NULL; set: both are needed; a
 *                          layer that is not trained: MPN_EINVAL naming the trained range; a set with rows pending: MPN_ESTATE.
 *                          mpn_mpnet_train_scale_momentum scales these buffers too.
 * The step for k > 0, in section 13.9's notation — B pending rows of I images, gm_t the (unmasked) gradient at tower t's mix output, y_t the
 * stored operand, c5 the last conv layer's channels, PP = PH * PW.  Only slab 0 of every operand, the conv5 slab (columns [0, c5) of
 * Kcat_t), gets a gradient: the conv4 / conv3 slabs' and the layers below the last pooling layer are not trained.
 *   1. gx_t[(bin,m), c] = sum_n gm_t[(bin,m), n] Wmix_t[n, c], c < c5, on the valid rows (PP segments of B rows at pitch Mp; the rows
 *      between two segments may hold anything, NaN included: they reach no valid result), n ascending in the order of the Linear layers'
 *      input gradient (four contiguous ranges of n, each ascending in pairs, their sums added in range order), before any weight is
 *      updated.  It is that kernel itself, run once per tower over the rows from the first segment's first to the last segment's last.
 *   2. nn.Normalize(2) x 1000 backward per (row, tower): with x the c5 * PP pooled values, s = 1000 / sqrt(sum x^2 + 1e-10) and
 *      y = s x the stored operand,  dx = s * (gx - y * (y . gx) / 1000^2).  Both sums (x . x for s, y . gx) run over the entries
 *      e = (c / 8 * PP + bin) * 8 + c % 8 in ONE order that depends on (c5, PP) alone: 256 partial sums, partial t taking the entries
 *      e = t, t + 256, t + 512, .. ascending from +0.0 with one fused multiply-add each, then the tree
 *      for (h = 128; h >= 1; h /= 2) part[t] += part[t + h] for t < h.  s is recomputed from x, which mpn_mpnet_train_add keeps beside the
 *      argmax; the training forward's bits are untouched.  conv345_unnormalized: dx = gx (the conv5 factor is 1).
 *   3. argmax, per Foveal region used, pending row, channel and bin: the FIRST strict maximum of the bin's window in row-major scan, -1 for
 *      an empty window (the ROI pooling's own rule), written by mpn_mpnet_train_add behind the pending rows; towers that pool the same
 *      region share it.  The forward keeps pooling from the range-max tables.
 *   4. the gradient map of image i at the last conv layer's output: per cell (c, y, x) ONE fp32 chain from +0.0 — towers ascending, inside a
 *      tower the image's rows ascending, inside a row the bins ascending, each term adding dx_t[n, c, bin] wherever
 *      argmax_t[n, c, bin] == y * W + x.  No atomics; every interior cell is written, the halo is zero.  Then the mask [conv5 output > 0]:
 *      nn.Normalize sits between the pooling and the ReLU, so the gradient at a pooled zero is not zero until here.
 *   5. the chain of MPN_TRAIN_CONV(k) above, layer by layer in its orders: db, dW, the input gradient (here always on the direct
 *      convolution kernel, never the Winograd one: DESIGN.md section 13.15) masked with the ReLU of the layer below, summed over
 *      the images in train_add order; optim.sgd on the master pack, then the Winograd pack (and a first layer's
 *      K = 36 pack) rebuilt in place — the forms a MultiPathNet handle's creation derives from the conv weights are the plain handle's —,
 *      so that every form is bit-identical to what creation builds from mpn_mpnet_get_trunk_weights' output.  detect and captured graphs
 *      see the new weights at once.
 *   6. every input gradient of the step, the towers' and the convs', is computed before any update; the step is deterministic and
 *      bit-reproducible with dropout on or off.
 * mpn_mpnet_train_begin_conv(k > 0) allocates, all or nothing: per tower two [c5, PP, Mp] gradient slabs (one unnormalised), per region
 * used the raw pools and the argmax [max_rois, c5, PP], the rows' Foveal table, MPN_TRAIN_MAX_IMAGES gradient maps, and the conv block's
 * buffers as MPN_TRAIN_CONV(k) (the saved maps, two gradient maps, per layer momentum, gradient and the input gradient's packs).
 * Debug tensors after such a step, valid until the next mpn_mpnet_train_add: "tower_train_argmax.<region>" [B, c5, PH, PW] (item 3, as
 * floats), "tower_train_gx5.<t>" and "tower_train_dx5.<t>" [B, c5, PH, PW] (items 1 and 2 for tower t), "tower_train_g5.<i>" [c5, h, w]
 * (item 4's map of image i behind the mask), "tower_train_act.<i>.<j>" (the saved maps, as "train_act.<i>.<j>").
 * Not here: the conv layers below the last pooling layer and the conv4 / conv3 slabs' gradients (the rest of phase 2), ResNet / op-list
 * towers, MPN_FC_SPLIT3, more than one GPU. */
int mpn_mpnet_train_begin(mpn_frcnn *p, float momentum, float weight_decay, float bbox_weight);
int mpn_mpnet_train_begin_conv(mpn_frcnn *p, int conv_layers, float momentum, float weight_decay, float bbox_weight);
int mpn_mpnet_get_trunk_weights(mpn_frcnn *p, int layer, float *d_w /*[Cout,Cin,3,3]*/, float *d_b /*[Cout]*/, void *stream);
int mpn_mpnet_train_get_trunk_state(mpn_frcnn *p, int layer, float *d_v /*[Cout,Cin,3,3]*/, float *d_vb /*[Cout]*/, void *stream);
int mpn_mpnet_train_set_trunk_state(mpn_frcnn *p, int layer, const float *d_v, const float *d_vb, void *stream);
int mpn_mpnet_train_add(mpn_frcnn *p, const float *d_image, int H, int W, const float *d_rois /*[n,4]*/,
                        const float *d_gt /*[n,4]*/, const int *d_labels /*[n], 0 = background*/, int n, void *stream);
int mpn_mpnet_train_step(mpn_frcnn *p, float lr, float *d_loss /*[2]: cls, bbox*/, void *stream);
int mpn_mpnet_train_end(mpn_frcnn *p);
int mpn_mpnet_train_set_dropout(mpn_frcnn *p, float rate, long seed);
int mpn_mpnet_train_set_head(mpn_frcnn *p, int k);
int mpn_mpnet_get_tower_weights(mpn_frcnn *p, int t, float *d_mix_w, float *d_mix_b, float *d_fc6_w, float *d_fc6_b, float *d_fc7_w,
                                float *d_fc7_b, void *stream);
int mpn_mpnet_get_head_weights(mpn_frcnn *p, float *d_cls_w, float *d_cls_b, float *d_bbox_w, float *d_bbox_b, void *stream);
int mpn_mpnet_train_get_state(mpn_frcnn *p, int tower, float *d_mix_v, float *d_mix_vb, float *d_fc6_v, float *d_fc6_vb,
                              float *d_fc7_v, float *d_fc7_vb, void *stream);
int mpn_mpnet_train_set_state(mpn_frcnn *p, int tower, const float *d_mix_v, const float *d_mix_vb, const float *d_fc6_v,
                              const float *d_fc6_vb, const float *d_fc7_v, const float *d_fc7_vb, void *stream);
int mpn_mpnet_train_get_head_state(mpn_frcnn *p, float *d_cls_v, float *d_cls_vb, float *d_bbox_v, float *d_bbox_vb,
                                   long *h_step, void *stream);
int mpn_mpnet_train_set_head_state(mpn_frcnn *p, const float *d_cls_v, const float *d_cls_vb, const float *d_bbox_v,
                                   const float *d_bbox_vb, long step, void *stream);
int mpn_frcnn_train_scale_momentum(mpn_frcnn *p, float factor, void *stream);
int mpn_mpnet_train_scale_momentum(mpn_frcnn *p, float factor, void *stream);

/* Drawing a training minibatch's rows on the device: DataSetCOCO:attachProposals with its crowd branch
 * (DataSetJSON.lua:280-390) and BatchProviderROI's setupOne + selectBBoxesOne (BatchProviderROI.lua:39-49, 98-101) for ONE image — what
 * lies between an image's proposals and mpn_frcnn_train_add / mpn_mpnet_train_add.  One launch each, no atomics, every order fixed:
 * the same inputs, seed and draw give the same bits.  Boxes are (x1, y1, x2, y2) in the image's own coordinates; inputs are NaN-free.
 *   mpn_attach_proposals   rows = [gt ; proposals], m = g + n.  Per row, over the g GT boxes in order, utils.boxoverlap in fp32 in the
 *                          reference's operation order (w = x2 - x1 + 1, h = y2 - y1 + 1, inter = w * h, o = inter / (aarea + barea - inter),
 *                          o = 0 where w < 0 or h < 0): d_overlap = the maximum, d_corr = the FIRST maximum's 1-based index (0 where the
 *                          maximum is 0), d_label = d_gt_labels[corr - 1] (0 without one).  Then the crowd branch: utils.intersection =
 *                          inter / aarea over the n_crowd crowd boxes — WITHOUT the w < 0 / h < 0 zeroing, as utils.lua:131-148 writes it,
 *                          so a box off a crowd's corner (both negative) has a positive value —; a row >= g whose maximum over the crowds
 *                          is > 0.7f gets d_overlap = -1 (neither foreground nor background); GT rows are never masked; d_corr and
 *                          d_label stay as they are.  Outputs d_boxes [m,4], d_overlap [m], d_corr [m], d_label [m].  g == 0 is legal
 *                          (every overlap 0); a pointer may be NULL only where its count is 0; g + n <= 2^28.
 *   mpn_sample_rois        foreground = overlap >= fg_threshold, background = bg_lo <= overlap < bg_hi, each list in ascending row order;
 *                          d_counts[2] = (n_bg, n_fg).  fg_num = (int)(fg_fraction * batch_size) in double, bg_num = batch_size - fg_num;
 *                          r_bg = min(bg_num, n_bg) and r_fg = min(fg_num, n_fg) draws WITH replacement.  Draw i of set s (0 background,
 *                          1 foreground): word 0 of Philox4x32-10 with
 *                            key     = (seed & 0xffffffff, seed >> 32)
 *                            counter = (i, draw & 0xffffffff, 0x80000000 + s, draw >> 32)
 *                          (the high bit of counter word 2 keeps the stream apart from the dropout masks' under the same seed), mapped to
 *                          list index (uint64(word) * count) >> 32.  Rows 0 .. r_bg - 1 are the background draws, then r_fg foreground
 *                          ones: d_rois = the row's box, d_gt = zeros on background rows and d_boxes[corr - 1] on foreground ones,
 *                          d_labels = 0 / the row's label.  flip_width > 0: both tables through mpn_flip_boxes' formula at that width
 *                          (zeros included).  Nothing past row r = r_bg + r_fg <= batch_size is written.  m > 0.
 *   mpn_frcnn_train_add_sampled / mpn_mpnet_train_add_sampled   attach + sample into buffers of the training state, read the two counts
 *                          back into h_counts (a HOST pointer; one stream synchronisation), then: n_bg == 0 or n_fg == 0 adds NOTHING and
 *                          returns MPN_OK — the caller draws another image —; pending + r > max_rois returns MPN_EINVAL and changes nothing;
 *                          otherwise exactly mpn_frcnn_train_add / mpn_mpnet_train_add of the r rows, with flip != 0 on the mirrored image
 *                          (mpn_image_hflip) and the boxes flipped at width W.  The flip decision is the caller's.
 * MPN_EINVAL, named in mpn_last_error, before any launch: a NULL required pointer or a NULL pointer with a positive count; n, g or
 * n_crowd < 0; g + n == 0; batch_size <= 0; fg_fraction not a finite number in [0, 1]; a threshold that is not finite; bg_lo > bg_hi.
 * Not here: dataset / JSON loading, sampleAroundGTBoxes, the scale / aspect jitter of getImages, bbox regression statistics, and the
 * choice of the images of a minibatch. */
typedef struct { int batch_size; double fg_fraction; float fg_threshold, bg_lo, bg_hi; } mpn_roi_sampler;
int mpn_attach_proposals(const float *d_proposals /*[n,4]*/, int n, const float *d_gt /*[g,4]*/, const int *d_gt_labels /*[g]*/, int g,
                         const float *d_crowds /*[n_crowd,4]*/, int n_crowd,
                         float *d_boxes /*[g+n,4]*/, float *d_overlap /*[g+n]*/, int *d_corr /*[g+n]*/, int *d_label /*[g+n]*/, void *stream);
int mpn_sample_rois(const float *d_boxes, const float *d_overlap, const int *d_corr, const int *d_label, int m,
                    const mpn_roi_sampler *cfg, uint64_t seed, uint64_t draw, int flip_width,
                    float *d_rois /*[batch_size,4]*/, float *d_gt /*[batch_size,4]*/, int *d_labels /*[batch_size]*/, int *d_counts /*[2]: n_bg, n_fg*/, void *stream);
int mpn_frcnn_train_add_sampled(mpn_frcnn *p, const float *d_image, int H, int W,
                                const float *d_proposals, int n, const float *d_gt, const int *d_gt_labels, int g,
                                const float *d_crowds, int n_crowd, const mpn_roi_sampler *cfg,
                                uint64_t seed, uint64_t draw, int flip, int *h_counts /*[2]: n_bg, n_fg*/, void *stream);
int mpn_mpnet_train_add_sampled(mpn_frcnn *p, const float *d_image, int H, int W,
                                const float *d_proposals, int n, const float *d_gt, const int *d_gt_labels, int g,
                                const float *d_crowds, int n_crowd, const mpn_roi_sampler *cfg,
                                uint64_t seed, uint64_t draw, int flip, int *h_counts /*[2]: n_bg, n_fg*/, void *stream);

/* Captured launch graphs.  The kernel chains of the per-image path — the head (transform .. decode) and the tail (per-class NMS,
 * voting, top-k) of mpn_frcnn_test_one / _pipelined / _pipelined_host, and the bodies of mpn_frcnn_shard_head / _shard_nms /
 * _shard_finish — are captured with hipStreamBeginCapture once per (buffer pointers, H, W, N) and replayed with hipGraphLaunch: one host
 * call per segment instead of 30-60 kernel launches (Tester_FRCNN.lua:54-139 calls testOne in a loop over same-sized inputs).  Results are
 * bit-identical to the ordinary launches.  Caller-provided buffers are captured at their second sighting, so a host that passes the
 * same device buffers every image gets the replays and one that allocates fresh ones never pays for a capture; a graph is dropped when a
 * library buffer it references is replaced.  OFF by default — opt in with enable = 1 here or MPN_GRAPHS=1 in the environment: measured
 * on MI355X the host's enqueue time per image drops 6.5x (AlexNet 484 -> 74 us) while the device-side timeline, and so the proposals/s
 * of a device-bound loop, does not improve (-0.5 %): it frees the host thread, it does not speed up the GPU.  Profiling
 * (mpn_frcnn_set_profiling) suspends it. */
int mpn_frcnn_set_graphs(mpn_frcnn *p, int enable);
int mpn_frcnn_graph_stats(const mpn_frcnn *p, long *captures, long *replays);

/* Per-kernel-group timing with HIP events recorded on the launch stream (bench.py's roofline leg).
 * Tags index the arrays returned by mpn_frcnn_get_profile (accumulated ms and launch-group counts). */
enum {
  MPN_PROF_TRANSFORM = 0, MPN_PROF_CONV_WINO /* Winograd F(2x2,3x3) layers */, MPN_PROF_CONV_DIRECT /* direct implicit-GEMM layers */, MPN_PROF_POOL, MPN_PROF_ROIPOOL, MPN_PROF_FC6,
  MPN_PROF_FC7, MPN_PROF_HEADS, MPN_PROF_POST, MPN_PROF_SELECT, MPN_PROF_NMS, MPN_PROF_TOPK, MPN_PROF_NTAGS
};
int mpn_frcnn_set_profiling(mpn_frcnn *p, int enable);
int mpn_frcnn_get_profile(mpn_frcnn *p, double *ms, long *counts, int n_tags, int reset);

/* Intermediate activations for parity tests: name in {"conv5","pooled","fc7","cls","bbox_raw"}; tower models (MultiPathNet, the
 * ResNet / op-list tower forms) keep "bbox_raw", "cls_k" (the K integral classifiers' pre-softmax logits, [N, K * C] row-major) and
 * "cat" (the towers' outputs side by side, [N, towers * fc_dim]); plain ResNet / op-list models keep "cls", "fc7" (the head's
 * average-pooled features) and "bbox_raw"; a plain handle with K > 1 integral classifiers (mpn_frcnn_create_integral) keeps "cls_k"
 * ([N, K * C]) in place of "cls". */
int mpn_frcnn_debug_tensor(mpn_frcnn *p, const char *name, const float **d_ptr, size_t *n_elems);

#ifdef __cplusplus
}
#endif
#endif /* MPN_H */
