"""Cost of choosing one image's minibatch rows: attach_proposals + the ROI sampler for 2000 proposals x 20 GT
boxes x 2 crowd regions, batch 128 at fg_fraction 0.25 — what BatchProviderROI does per image of a Fast R-CNN minibatch.
  device  mpn_attach_proposals + mpn_sample_rois, inputs resident on the device: HIP events around --reps back-to-back pairs of
          launches (a window of many pairs: one pair is a few microseconds, far below an event's resolution), median over --steps
          windows after --warmup; and the same pair with the counts read back each time (what *_train_add_sampled pays: one
          synchronisation per image), on the host clock
  host    train.attach_proposals(crowd_boxes=...) + RoiSampler.sample in numpy, then the three arrays copied to the device (what
          train_add needs), host clock around work that ends in a synchronise; the process's thread limit is printed beside it
The two paths' rows differ (another generator); their record is checked equal first.  One JSON line per measurement.

    python tools/bench_sampler.py [--steps 20] [--warmup 5] [--reps 200]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 600, 1000


def image_case(rng, n=2000, g=20, n_classes=21):
    """one image's (proposals [n,4], gt [g,4], labels [g], crowds [2,4]): a quarter of the proposals jittered copies of GT boxes, a
    quarter copies shifted by 0.45 of the width, the rest anywhere; two crowd strips over the image's whole height"""
    x1, y1 = rng.uniform(1, W - 260, g), rng.uniform(1, H - 200, g)
    gt = np.stack([x1, y1, x1 + rng.uniform(40, 250, g), y1 + rng.uniform(40, 190, g)], 1).astype(np.float32)
    labels = rng.integers(1, n_classes, g).astype(np.int32)
    prop = np.zeros((n, 4), np.float32)
    for i in range(n):
        b = gt[i % g]
        if i % 4 == 0:
            prop[i] = b + rng.uniform(-4, 4, 4)
        elif i % 4 == 1:
            prop[i] = b + 0.45 * (b[2] - b[0]) * np.array([1, 0, 1, 0]) + rng.uniform(-2, 2, 4)
        else:
            c, wh = rng.uniform([40, 40], [W - 40, H - 40]), np.exp(rng.uniform(np.log(24), np.log(300), 2))
            prop[i] = np.concatenate([c - wh / 2, c + wh / 2])
    prop = np.clip(prop, 1, [W, H, W, H]).astype(np.float32)
    crowds = np.array([[W - 120, 0, W - 60, 2 * H], [300, 0, 330, 2 * H]], np.float32)
    return prop, gt, labels, crowds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200, help="launch pairs per timed window")
    a = ap.parse_args()
    import torch
    from multipathnet_amd import train
    assert torch.cuda.is_available(), "bench_sampler needs a HIP device"
    name = torch.cuda.get_device_name(0)
    prop, gt, gl, crowds = image_case(np.random.default_rng(5))
    n, g = len(prop), len(gt)
    d_prop, d_gt, d_gl, d_crowds = (torch.from_numpy(x).cuda() for x in (prop, gt, gl, crowds))
    rec = train.attach_proposals_device(d_prop, d_gt, d_gl, d_crowds)
    host = train.attach_proposals(prop, gt, gl, crowd_boxes=crowds)
    assert (rec["overlap"].cpu().numpy().view(np.uint32) == host["overlap"].view(np.uint32)).all(), "device and host records differ"
    assert (rec["correspondance"].cpu().numpy() == host["correspondance"]).all()
    smp = train.DeviceRoiSampler(128, 0.25, 0.5, (0.1, 0.5), seed=555)
    smp.sample(rec, 0)
    shape = {"proposals": n, "gt": g, "crowds": len(crowds), "batch_size": 128, "n_bg": smp.counts[0], "n_fg": smp.counts[1], "masked": int((host["overlap"] == -1).sum())}

    # ---- device: the two launches, events around a window of back-to-back pairs
    lib = __import__("multipathnet_amd").load()
    cfg = smp.cfg()
    out = [torch.empty((128, 4), device="cuda"), torch.empty((128, 4), device="cuda"), torch.empty(128, dtype=torch.int32, device="cuda"),
           torch.empty(2, dtype=torch.int32, device="cuda")]
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def pair(draw):
        rc = lib.mpn_attach_proposals(p(d_prop), n, p(d_gt), p(d_gl), g, p(d_crowds), len(crowds), p(rec["boxes"]), p(rec["overlap"]),
                                      p(rec["correspondance"]), p(rec["label"]), s)
        rc = rc or lib.mpn_sample_rois(p(rec["boxes"]), p(rec["overlap"]), p(rec["correspondance"]), p(rec["label"]), n + g, C.byref(cfg), 555, draw, 0,
                                       p(out[0]), p(out[1]), p(out[2]), p(out[3]), s)
        assert rc == 0, lib.mpn_last_error()

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for i in range(a.warmup + a.steps):
        e0.record()
        for r in range(a.reps):
            pair(i * a.reps + r)
        e1.record()
        e1.synchronize()
        if i >= a.warmup:
            us.append(e0.elapsed_time(e1) * 1e3 / a.reps)
    print(json.dumps(dict(shape, what="device_attach_plus_sample", method="HIP events around %d back-to-back launch pairs" % a.reps,
                          us_per_image_median=round(float(np.median(us)), 2), us_per_image_min=round(float(np.min(us)), 2),
                          us_per_image_max=round(float(np.max(us)), 2), windows=a.steps, device=name)), flush=True)
    us = []
    for i in range(a.warmup + a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for r in range(a.reps):
            pair(i * a.reps + r)
            out[3].cpu()   # the counts back: the one synchronisation per image
        us.append((time.perf_counter() - t0) * 1e6 / a.reps)
    us = us[a.warmup:]
    print(json.dumps(dict(shape, what="device_attach_plus_sample_with_count_readback", method="host clock, %d pairs per window, each ending in the 8-byte readback" % a.reps,
                          us_per_image_median=round(float(np.median(us)), 2), us_per_image_min=round(float(np.min(us)), 2),
                          us_per_image_max=round(float(np.max(us)), 2), windows=a.steps, device=name)), flush=True)

    # ---- host: numpy attach + sample, then the rows to the device
    host_smp = train.RoiSampler(128, 0.25, 0.5, (0.1, 0.5), rng=np.random.default_rng(555))
    reps = max(1, a.reps // 20)
    us = []
    for i in range(a.warmup + a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for r in range(reps):
            hrec = train.attach_proposals(prop, gt, gl, crowd_boxes=crowds)
            rows = host_smp.sample(hrec)
            dev_rows = [torch.from_numpy(x).cuda() for x in rows]
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6 / reps)
    us = us[a.warmup:]
    assert dev_rows[0].shape[0] > 0
    print(json.dumps(dict(shape, what="host_attach_plus_sample_plus_upload", method="host clock around %d images ending in a synchronise" % reps,
                          us_per_image_median=round(float(np.median(us)), 1), us_per_image_min=round(float(np.min(us)), 1),
                          us_per_image_max=round(float(np.max(us)), 1), windows=a.steps, host_threads=torch.get_num_threads(),
                          omp_num_threads=os.environ.get("OMP_NUM_THREADS"), device=name)), flush=True)


if __name__ == "__main__":
    main()
