"""COCOeval (bbox) at val2017 size: device time of mpn_coco_eval_run (evaluate + accumulate) against the numpy restatement.

A seeded synthetic set: 5 000 images, COCO's 80 sparse category ids, ~7.3 GTs per image (1 % crowd, `area` independent of the
box), 100 detections per image (~half of them jittered GTs).  Device time: HIP events around the call after warm-up, median of
--reps.  CPU time: tests/cocoeval_np.py (the restatement the tests compare against) on the same rows, once.  The per-kernel split
comes from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/bench_cocoeval.py --no-cpu`.

    python tools/bench_cocoeval.py [--images 5000] [--reps 20] [--no-cpu] [--check]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2017)
    ap.add_argument("--no-cpu", action="store_true", help="skip the numpy restatement")
    ap.add_argument("--check", action="store_true", help="assert device == restatement (implies the CPU run)")
    a = ap.parse_args()
    import cocoeval_np as R
    gt, rows = R.synthetic(a.seed, a.images, R.COCO_CAT_IDS, gt_per_img=7.3, det_per_img=a.dets, crowd=0.01)
    out = {"images": a.images, "categories": len(R.COCO_CAT_IDS), "gts": int(gt["id"].size), "rows": int(rows.shape[0])}
    import torch
    from multipathnet_amd.cocoeval import COCOEvaluator
    assert torch.cuda.is_available(), "bench_cocoeval needs a HIP device"
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    ev = COCOEvaluator(gt, device=dev)
    out["create_s"] = round(time.perf_counter() - t0, 3)
    d_rows = torch.from_numpy(rows).to(dev)
    for _ in range(a.warmup):
        ev.run(d_rows)
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ev.run(d_rows)         # evaluate + accumulate on the device (the arrays stay there)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    t0 = time.perf_counter()
    res = ev.evaluate(d_rows)
    out["evaluate_with_copy_back_s"] = round(time.perf_counter() - t0, 4)
    out["device_ms_median"] = round(float(np.median(ms)), 3)
    out["device_ms_min"] = round(float(np.min(ms)), 3)
    out["device_ms_max"] = round(float(np.max(ms)), 3)
    out["reps"] = a.reps
    out["stats"] = [round(float(s), 6) for s in res["stats"]]
    if a.check or not a.no_cpu:
        t0 = time.perf_counter()
        ref = R.evaluate(gt, rows)
        out["numpy_cpu_s"] = round(time.perf_counter() - t0, 2)
        same = all(np.array_equal(res[k], ref[k]) for k in ("precision", "recall", "scores"))
        out["equal_to_restatement"] = bool(same)
        if a.check:
            assert same
    ev.summarize()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
