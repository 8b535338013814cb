"""Cost of horizontal-flip test-time augmentation on one GPU: VGG-16 Fast R-CNN on bench.synthetic_inputs()
(600 x 1000, 1000 ROIs), ms/image from HIP events (median of --steps after --warmup) for
  plain:     mpn_frcnn_test_one without augmentation (the headline setting);
  augmented: mpn_frcnn_test_one after mpn_frcnn_set_augment(1);
  two_calls: what a caller had to do for the same detections before the setter existed — two mpn_frcnn_detect calls (the image and
             its mirror, the mirror and the flipped boxes prepared once outside the timed region), the two table pairs copied to the
             host, merged there in numpy, uploaded, then the tail through the module-level entries (select, batched NMS, top-k).
The trunk / head / tail split of the first two comes from mpn_frcnn_set_profiling in a separate pass.  One JSON line per setting; the
program fails if `two_calls` and `augmented` disagree in a single bit of the detection record.

    python tools/bench_augment.py [--steps 20] [--warmup 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPS = {"trunk": ("transform", "conv_wino", "conv_direct", "pool"), "head": ("roi_pool", "fc6", "fc7", "heads", "post"),
          "tail": ("select", "nms", "topk")}
F32 = np.float32


def _flip(b, W):
    out = b.copy()
    out[:, 0] = ((-b[:, 2]) + F32(W)) + F32(1)
    out[:, 2] = ((-b[:, 0]) + F32(W)) + F32(1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    import bench
    from multipathnet_amd import _lib, models, utils
    from multipathnet_amd.nn import _f, _i, _stream
    assert torch.cuda.is_available(), "bench_augment needs a HIP device"
    P = models.synthetic_params(seed=557)
    im, boxes = bench.synthetic_inputs()
    H, W = im.shape[1:]
    N = boxes.shape[0]
    d_im, d_bx = torch.from_numpy(im).cuda(), torch.from_numpy(boxes).cuda()
    d_imf, d_bxf = torch.from_numpy(np.ascontiguousarray(im[..., ::-1])).cuda(), torch.from_numpy(_flip(boxes, W)).cuda()
    net = models.FastRCNN(P, max_h=H, max_w=W, max_rois=N)
    lib = _lib.load()

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(a.steps):
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"ms_per_image_median": round(float(np.median(ms)), 3), "ms_min": round(float(np.min(ms)), 3), "ms_max": round(float(np.max(ms)), 3)}

    def profiled():
        net.set_profiling(True)
        net.get_profile(reset=True)
        k = 5
        for _ in range(k):
            net.test_one_async(d_im, d_bx)
        prof = net.get_profile(reset=True)
        net.set_profiling(False)
        out = {g: round(sum(prof[t][0] for t in tags) / k, 3) for g, tags in GROUPS.items()}
        out["by_tag"] = {t: round(prof[t][0] / k, 3) for t in net.PROF_TAGS if prof[t][1]}
        return out

    def two_calls():
        sA, bA = net.detect(d_im, d_bx, clamp=False)
        sB, bB = net.detect(d_imf, d_bxf, clamp=False)
        sA, bA, sB, bB = [t.cpu().numpy() for t in (sA, bA, sB, bB)]
        sc = (sA + sB) * F32(0.5)
        bb = ((bA + _flip(bB.reshape(-1, 4), W).reshape(bB.shape)) * F32(0.5)).reshape(-1, 4)
        bb[:, 0::2] = np.where(bb[:, 0::2] < 1, F32(1), np.where(bb[:, 0::2] > W, F32(W), bb[:, 0::2]))
        bb[:, 1::2] = np.where(bb[:, 1::2] < 1, F32(1), np.where(bb[:, 1::2] > H, F32(H), bb[:, 1::2]))
        d_sc, d_bb = torch.from_numpy(sc).cuda(), torch.from_numpy(bb.reshape(bA.shape)).cuda()
        Cc = sc.shape[1]
        scored = torch.empty((Cc - 1, N, 5), dtype=torch.float32, device=d_sc.device)
        counts = torch.zeros(Cc - 1, dtype=torch.int32, device=d_sc.device)
        _lib.check(lib.mpn_select_scored(_f(d_sc), _f(d_bb), N, Cc, 1, C.c_float(-1.5), _f(scored), _i(counts), None, _stream()), "select_scored")
        keep, _, n_keep = utils.nms_batched(scored, counts, 0.3)
        out = torch.empty((net._dets.size(0), 6), dtype=torch.float32, device=d_sc.device)
        thr = torch.zeros(1, dtype=torch.float32, device=d_sc.device)
        n_out = torch.zeros(1, dtype=torch.int32, device=d_sc.device)
        _lib.check(lib.mpn_keep_top_k(_f(keep), _i(n_keep), Cc - 1, N, 100, _f(thr), _f(out), out.size(0), _i(n_out), _stream()), "keep_top_k")
        return out, n_out

    base = {"n_rois": int(N), "image": "%dx%d" % (H, W), "steps": a.steps, "device": torch.cuda.get_device_name(0)}
    r = timed(lambda: net.test_one_async(d_im, d_bx))
    r.update(setting="plain", profiled_ms_per_image=profiled(), **base)
    print(json.dumps(r), flush=True)
    r = timed(two_calls)
    r.update(setting="two_calls", **base)
    print(json.dumps(r), flush=True)
    ref, n_ref = two_calls()
    torch.cuda.synchronize()
    net.set_augment(True)
    r = timed(lambda: net.test_one_async(d_im, d_bx))
    r.update(setting="augmented", profiled_ms_per_image=profiled(), **base)
    print(json.dumps(r), flush=True)
    d, n = net.test_one_async(d_im, d_bx)
    torch.cuda.synchronize()
    k = int(n.item())
    rows = lambda t: sorted(map(tuple, t[:k].cpu().numpy().view(np.uint32).tolist()))   # the same rows, whatever the record's order
    assert k == int(n_ref.item()) and k > 0 and rows(d) == rows(ref), "augmented test_one and the two-call construction disagree"
    net.close()


if __name__ == "__main__":
    main()
