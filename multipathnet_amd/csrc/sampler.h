// sampler.h — internal interface of the minibatch sampler (sampler.hip): DataSetCOCO:attachProposals and BatchProviderROI's setupOne +
// selectBBoxesOne for one image on the device.  Used by mpn_attach_proposals / mpn_sample_rois (sampler.hip) and by the two
// *_train_add_sampled entry points (train_driver.hip).  include/mpn.h states the contract; DESIGN.md section 13.11.
#pragma once
#include "mpn_internal.h"

namespace mpn {

// The refusals every entry point that takes these arguments shares: MPN_EINVAL with the argument named in mpn_last_error under `fn`, before
// anything touches the device.
int check_attach_args(const char *fn, const float *d_proposals, int n, const float *d_gt, const int *d_gt_labels, int g, const float *d_crowds,
                      int n_crowd);
int check_sampler_cfg(const char *fn, const mpn_roi_sampler *cfg, int flip_width);

// attach_proposals_kernel, one launch: rows [gt ; proposals], m = g + n.  Arguments checked by the caller (check_attach_args).
int attach_proposals(const float *d_proposals, int n, const float *d_gt, const int *d_gt_labels, int g, const float *d_crowds, int n_crowd,
                     float *d_boxes, float *d_overlap, int *d_corr, int *d_label, hipStream_t s);
// roi_sample_kernel, one launch of one block.  d_lists: 2 * m ints of scratch (the background and the foreground row lists).  At most
// cfg.batch_size rows of d_rois / d_gt / d_labels are written; d_counts[2] = (n_bg, n_fg).
int roi_sample(const float *d_boxes, const float *d_overlap, const int *d_corr, const int *d_label, int m, const mpn_roi_sampler &cfg,
               uint64_t seed, uint64_t draw, int flip_width, int *d_lists, float *d_rois, float *d_gt, int *d_labels, int *d_counts, hipStream_t s);
// (int)(fg_fraction * batch_size) in double (BatchProviderROI.lua:116)
inline int sampler_fg_num(const mpn_roi_sampler &cfg) { return (int)(cfg.fg_fraction * (double)cfg.batch_size); }

}  // namespace mpn
