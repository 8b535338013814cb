"""Cost of multi-scale testing on one GPU: VGG-16 Fast R-CNN on bench.synthetic_inputs() with 1000 ROIs at
  S = 1: 600, max 1000 (the headline setting);
  S = 5: Fast R-CNN's {480, 576, 688, 864, 1200}, max 1000 (canvas 600 x 1000, three distinct levels);
  S = 5: the same targets, max 2000 (canvas 1200 x 2000, five levels).
ms/image of mpn_frcnn_test_one from HIP events (median of --steps after --warmup), then the trunk / head / tail split from
mpn_frcnn_set_profiling in a separate pass.  One JSON line per setting.

    python tools/bench_multiscale.py [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRCNN_TARGETS = [480, 576, 688, 864, 1200]
SETTINGS = [("S1_600_max1000", [600], 1000, 600, 1000), ("S5_max1000", FRCNN_TARGETS, 1000, 600, 1000),
            ("S5_max2000", FRCNN_TARGETS, 2000, 1200, 2000)]
GROUPS = {"trunk": ("transform", "conv_wino", "conv_direct", "pool"), "head": ("roi_pool", "fc6", "fc7", "heads", "post"),
          "tail": ("select", "nms", "topk")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    import bench
    from multipathnet_amd import models
    assert torch.cuda.is_available(), "bench_multiscale needs a HIP device"
    P = models.synthetic_params(seed=557)
    im, boxes = bench.synthetic_inputs()
    d_im, d_bx = torch.from_numpy(im).cuda(), torch.from_numpy(boxes).cuda()
    for name, targets, max_size, mh, mw in SETTINGS:
        net = models.FastRCNN(P, max_h=mh, max_w=mw, max_rois=boxes.shape[0], scale=targets, max_size=max_size)
        for _ in range(a.warmup):
            net.test_one_async(d_im, d_bx)
        torch.cuda.synchronize()
        ms = []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(a.steps):
            e0.record()
            net.test_one_async(d_im, d_bx)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        net.set_profiling(True)
        net.get_profile(reset=True)
        k = 5
        for _ in range(k):
            net.test_one_async(d_im, d_bx)
        prof = net.get_profile(reset=True)
        net.set_profiling(False)
        split = {g: round(sum(prof[t][0] for t in tags) / k, 3) for g, tags in GROUPS.items()}
        print(json.dumps({"setting": name, "targets": targets, "max_size": max_size, "n_rois": int(boxes.shape[0]),
                          "ms_per_image_median": round(float(np.median(ms)), 3), "ms_min": round(float(np.min(ms)), 3),
                          "ms_max": round(float(np.max(ms)), 3), "steps": a.steps, "profiled_ms_per_image": split,
                          "device": torch.cuda.get_device_name(0)}), flush=True)
        net.close()


if __name__ == "__main__":
    main()
