"""Cost of one training step of the Fast R-CNN head on one GPU: VGG-16 at 600 x 1000, the reference's minibatch
of 2 images x 64 ROIs (BatchProviderROI.lua:18-24 with 128 rows in all), frozen trunk.
Per depth (0 = cls + bbox, 1 = + fc7, 2 = + fc6, 3 / 4 / 5 = + conv5_3 / conv5_2 / conv5_1): ms of mpn_frcnn_train_step alone and of the whole iteration (two train_add — trunk,
projection, ROI pooling each — plus the step), HIP events, median of --steps after --warmup.  Then fc6's fused weight-gradient + SGD
kernel alone (debug flavour, mpn_debug_bench_train_fc6: back-to-back launches) and its GB/s against the bytes it must move — the packed
weights and their momentum, each read and written once — and, at depth 3, the conv weight-gradient kernel alone on conv5_3 (512 -> 512 at
38 x 63, mpn_debug_bench_train_wgrad) against its floor: 2 * 9 * 512 * 512 * 38 * 63 = 11.3 GFLOP at the fp32 MFMA peak of 157.3 TFLOP/s.
--trunk-layers k adds, after the depths above, the depth MPN_TRAIN_TRUNK(k) — k = 9 is the reference's conv3_1
and up, through two pooling layers — with the same two numbers, and the max-pool backward kernel alone on the largest pooled trained layer
(k = 9: conv3_3, 256 x 150 x 250; mpn_debug_bench_train_poolbwd) against the bytes it must move: X and dX once each, dY once, at the
6.3 TB/s a float4 copy reaches.
--dropout RATE runs every step with nn.Dropout(RATE) behind fc6 and fc7 (0.5: the reference's default; two
more small kernels per step and a scale in two input gradients); 0, the default, launches nothing more than a run without the option.
--integral K trains a handle with the integral loss's K classifiers (models.integral_params: a fused head of
(K + 4) C rows instead of 5 C), step i on head i mod K as the reference's K donkeys take turns; 1, the default, is the plain handle.
--model mpnet measures instead the tower training of a MultiPathNet handle (models.synthetic_mpnet_params: VGG-16,
the five MPN_TOWERS, fc_dim 4096, C 81, K 6; mpn_mpnet_train_*): ms of mpn_mpnet_train_step alone and of the whole iteration on the same
2 x 64 rows, step i on classifier i mod K, beside the step's derived floor — every trained weight and its momentum read and written once.
--conv-layers k with it also trains the trunk's last k conv layers through the towers' skip pooling (3: conv5_1 ..
conv5_3): the same two times; 0, the default, is the tower training above.
--device-sampler measures instead the whole iteration at depth 2 with each image's rows chosen from 2000
proposals, drawn on the device (train_add_sampled) and, alternating in the same run, on the host (numpy + uploads + train_add).
--scale-momentum measures instead the learning-rate drop's momentum scaling per call — the VGG-16 towers and the
plain handle at MPN_TRAIN_TRUNK(--trunk-layers, 9 without it) — beside its HBM floor and beside get -> multiply -> set on the plain handle.
One JSON line per measurement.

    python tools/bench_train.py [--steps 20] [--warmup 5] [--trunk-layers 9] [--dropout 0.5] [--integral 6] [--model mpnet [--conv-layers 3]] [--device-sampler]
                                [--scale-momentum]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, ROWS, IMAGES = 600, 1000, 64, 2


def batch(rng, n_classes):
    im = rng.random((3, H, W), dtype=np.float32)
    c = rng.uniform([40, 40], [W - 40, H - 40], (ROWS, 2))
    wh = np.exp(rng.uniform(np.log(32), np.log(300), (ROWS, 2)))
    rois = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 1, [W, H, W, H]).astype(np.float32)
    gt = (rois + rng.normal(0, 2.0, (ROWS, 4))).astype(np.float32)
    labels = rng.integers(1, n_classes, ROWS).astype(np.int32)
    labels[: ROWS * 3 // 4] = 0   # fg_fraction 0.25, background rows first
    return im, rois, gt, labels


def bench_mpnet(a):
    """mpn_mpnet_train_step and the whole iteration (two tower_train_add + the step) on the product library"""
    import torch
    from multipathnet_amd import models
    P = models.synthetic_mpnet_params(seed=557)
    K, C_ = P["n_integral"], P["n_classes"]
    rng = np.random.default_rng(5)
    dev_batches = [[torch.from_numpy(x).cuda() for x in batch(rng, C_)] for _ in range(IMAGES)]
    net = models.MultiPathNet(P, max_h=H, max_w=W, max_rois=IMAGES * ROWS)
    trained = sum(int(T[k].numel()) for T in P["towers"] for k in ("mix_w", "mix_b", "fc6_w", "fc6_b", "fc7_w", "fc7_b")) + \
        sum(int(P[k].numel()) for k in ("cls_w", "cls_b", "bbox_w", "bbox_b"))
    gb = 4 * trained * 4 / 1e9   # w read + w write + v read + v write
    del P
    net.tower_train_begin(momentum=0.9, weight_decay=5e-4, dropout=a.dropout, conv_layers=a.conv_layers)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    step_ms, iter_ms = [], []
    for i in range(a.warmup + a.steps):
        e[0].record()
        for b in dev_batches:
            net.tower_train_add(*b)
        e[1].record()
        net.tower_train_set_head(i % K)
        net.tower_train_step(1e-6)   # a tiny step: the weights stay in their range over the run
        e[2].record()
        e[2].synchronize()
        if i >= a.warmup:
            step_ms.append(e[1].elapsed_time(e[2]))
            iter_ms.append(e[0].elapsed_time(e[2]))
    net.tower_train_end()
    net.close()
    print(json.dumps({"what": "mpnet_train_step", "towers": 5, "conv_layers": a.conv_layers, "dropout": a.dropout, "integral": K, "rows": IMAGES * ROWS,
                      "ms_step_median": round(float(np.median(step_ms)), 3), "ms_step_min": round(float(np.min(step_ms)), 3),
                      "ms_iteration_median": round(float(np.median(iter_ms)), 3), "gbytes_weights_and_momentum": round(gb, 2),
                      "floor_ms_at_6.3TBps": round(gb / 6.3e3 * 1e3, 3), "steps": a.steps, "device": torch.cuda.get_device_name(0)}), flush=True)


def bench_sampled(a):
    """--device-sampler: the whole iteration at depth 2 with each image's rows chosen from 2000 proposals x 20 GT boxes x 2 crowds
    (tools/bench_sampler.py's image), batch 64 per image — drawn on the device by train_add_sampled, against the host-sampled run of
    the same build (train.attach_proposals + RoiSampler.sample in numpy, three uploads, train_add).  Host clock around iterations that
    end in a synchronise: the host's work is what differs."""
    import time
    import torch
    from multipathnet_amd import models, train
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from bench_sampler import image_case
    P = models.synthetic_params(seed=557)
    C_ = P["cls_w"].shape[0]
    rng = np.random.default_rng(5)
    images = []
    for _ in range(IMAGES):
        prop, gt, gl, crowds = image_case(rng, n_classes=C_)
        images.append(dict(im=torch.from_numpy(rng.random((3, H, W), dtype=np.float32)).cuda(), host=(prop, gt, gl, crowds),
                           dev=[torch.from_numpy(x).cuda() for x in (prop, gt, gl, crowds)]))
    net = models.FastRCNN(P, max_h=H, max_w=W, max_rois=IMAGES * ROWS)
    del P
    dev_smp = train.DeviceRoiSampler(ROWS, 0.25, 0.5, (0.1, 0.5), seed=555)
    host_smp = train.RoiSampler(ROWS, 0.25, 0.5, (0.1, 0.5), rng=np.random.default_rng(555))

    def host_iter(i):
        for im in images:
            prop, gt, gl, crowds = im["host"]
            rows = host_smp.sample(train.attach_proposals(prop, gt, gl, crowd_boxes=crowds))
            net.train_add(im["im"], *[torch.from_numpy(x).cuda() for x in rows])

    def dev_iter(i):
        for j, im in enumerate(images):
            prop, gt, gl, crowds = im["dev"]
            n_bg, n_fg = net.train_add_sampled(im["im"], prop, gt, gl, dev_smp, draw=i * IMAGES + j, crowd_boxes=crowds)
            assert n_bg and n_fg

    net.train_begin(depth=2, momentum=0.9, weight_decay=5e-4, dropout=a.dropout)
    ms = {"host": [], "device": []}
    for i in range(a.warmup + a.steps):
        for which, fn in (("host", host_iter), ("device", dev_iter)):   # alternating: both see the same machine state
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(i)
            net.train_step(1e-6)
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms[which].append((time.perf_counter() - t0) * 1e3)
    net.train_end()
    net.close()
    for which in ("host", "device"):
        v = ms[which]
        print(json.dumps({"what": "train_iteration_%s_sampler" % which, "depth": 2, "dropout": a.dropout, "images": IMAGES, "rows_per_image": ROWS,
                          "proposals": 2000, "gt": 20, "crowds": 2, "ms_iteration_median": round(float(np.median(v)), 3),
                          "ms_iteration_min": round(float(np.min(v)), 3), "ms_iteration_max": round(float(np.max(v)), 3), "steps": a.steps,
                          "host_threads": torch.get_num_threads(), "device": torch.cuda.get_device_name(0)}), flush=True)


def bench_scale(a):
    """--scale-momentum: *_train_scale_momentum per call — the learning-rate drop's dfdx:mul(decay), DESIGN.md section 13.13 — on the
    VGG-16 towers and on the plain handle at MPN_TRAIN_TRUNK(k) (k = --trunk-layers, 9 without it): HIP events around a window of
    --steps calls after --warmup, beside the floor — every momentum byte read and written once at 6.3 TB/s — and, on the plain handle,
    the only alternative a host had before: train_state() -> multiply -> train_load_state()."""
    import torch
    from multipathnet_amd import models
    name = torch.cuda.get_device_name(0)

    def window(fn):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for _ in range(a.warmup):
            fn()
        e[0].record()
        for _ in range(a.steps):
            fn()
        e[1].record()
        e[1].synchronize()
        return e[0].elapsed_time(e[1]) / a.steps

    def numel(S):
        flat = []
        for v in S.values():
            if isinstance(v, dict):
                flat += list(v.values())
            elif isinstance(v, list):
                for x in v:
                    flat += list(x.values()) if isinstance(x, dict) else [x]
            else:
                flat.append(v)
        return sum(int(x.numel()) for x in flat if isinstance(x, torch.Tensor))

    def report(what, ms, n, **kw):
        gb = 2 * 4 * n / 1e9   # read + write
        print(json.dumps(dict({"what": what, "ms_per_call": round(ms, 4), "momentum_elements": n, "gbytes_moved": round(gb, 3),
                               "gbytes_per_s": round(gb / (ms * 1e-3), 1), "floor_ms_at_6.3TBps": round(gb / 6.3e3 * 1e3, 4), "calls": a.steps,
                               "device": name}, **kw)), flush=True)

    P = models.synthetic_mpnet_params(seed=557)
    net = models.MultiPathNet(P, max_h=H, max_w=W, max_rois=IMAGES * ROWS)
    del P
    net.tower_train_begin(momentum=0.9, weight_decay=5e-4)
    n = numel(net.tower_train_state())
    report("mpnet_train_scale_momentum", window(lambda: net.tower_train_scale_momentum(0.5)), n, towers=5)
    net.tower_train_end()
    net.close()
    del net
    torch.cuda.empty_cache()

    k = a.trunk_layers or 9
    net = models.FastRCNN(models.synthetic_params(seed=557), max_h=H, max_w=W, max_rois=IMAGES * ROWS)
    net.train_begin(trunk_layers=k, momentum=0.9, weight_decay=5e-4)
    n = numel(net.train_state())
    report("frcnn_train_scale_momentum", window(lambda: net.train_scale_momentum(0.5)), n, depth="MPN_TRAIN_TRUNK(%d)" % k)

    def get_multiply_set():
        S = net.train_state()
        mul = lambda v: v * 0.5 if isinstance(v, torch.Tensor) else v
        S = {key: ([mul(x) for x in v] if isinstance(v, list) else mul(v)) for key, v in S.items()}
        net.train_load_state(S)

    report("frcnn_get_multiply_set", window(get_multiply_set), n, depth="MPN_TRAIN_TRUNK(%d)" % k)
    net.train_end()
    net.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale-momentum", action="store_true", help="instead: *_train_scale_momentum per call on both models, and get -> multiply -> set on the plain handle")
    ap.add_argument("--device-sampler", action="store_true", help="instead: the iteration with the rows drawn on the device (train_add_sampled) against the host-sampled one")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trunk-layers", type=int, default=0, help="also measure MPN_TRAIN_TRUNK(k) (9: conv3_1 and up, the reference's configuration)")
    ap.add_argument("--dropout", type=float, default=0.0, help="dropout rate behind fc6 / fc7 (0.5: the reference's default; 0: none)")
    ap.add_argument("--integral", type=int, default=1, help="K classifiers of the integral loss, trained in turn (6: the reference's scripts; 1: the plain head)")
    ap.add_argument("--conv-layers", type=int, default=0, help="--model mpnet: also train the trunk's last k conv layers through the skip pooling (3: conv5_1 .. conv5_3)")
    ap.add_argument("--model", choices=("vgg", "mpnet"), default="vgg", help="mpnet: the tower training of a MultiPathNet handle (mpn_mpnet_train_*)")
    a = ap.parse_args()
    import torch
    from multipathnet_amd import _lib, models
    assert torch.cuda.is_available(), "bench_train needs a HIP device"
    if a.scale_momentum:
        return bench_scale(a)
    if a.device_sampler:
        return bench_sampled(a)
    if a.model == "mpnet":
        return bench_mpnet(a)
    P = models.synthetic_params(seed=557)
    C_ = P["cls_w"].shape[0]
    if a.integral > 1:
        P = models.integral_params(P, a.integral)
    rng = np.random.default_rng(5)
    dev_batches = [[torch.from_numpy(x).cuda() for x in batch(rng, C_)] for _ in range(IMAGES)]
    name = torch.cuda.get_device_name(0)
    with _lib.debug_hooks() as lib:
        net = models.FastRCNN(P, max_h=H, max_w=W, max_rois=IMAGES * ROWS)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        for depth in (0, 1, 2, 3, 4, 5) + (("trunk",) if a.trunk_layers > 0 else ()):
            if depth == "trunk":
                net.train_begin(trunk_layers=a.trunk_layers, momentum=0.9, weight_decay=5e-4, dropout=a.dropout)
            else:
                net.train_begin(depth=depth, momentum=0.9, weight_decay=5e-4, dropout=a.dropout)
            step_ms, iter_ms = [], []
            for i in range(a.warmup + a.steps):
                e[0].record()
                for b in dev_batches:
                    net.train_add(*b)
                e[1].record()
                if a.integral > 1:
                    net.train_set_head(i % a.integral)
                net.train_step(1e-6)   # a tiny step: the weights stay in their range over the run
                e[2].record()
                e[2].synchronize()
                if i >= a.warmup:
                    step_ms.append(e[1].elapsed_time(e[2]))
                    iter_ms.append(e[0].elapsed_time(e[2]))
            print(json.dumps({"what": "train_step", "depth": "MPN_TRAIN_TRUNK(%d)" % a.trunk_layers if depth == "trunk" else depth, "dropout": a.dropout, "integral": a.integral, "rows": IMAGES * ROWS, "ms_step_median": round(float(np.median(step_ms)), 3),
                              "ms_step_min": round(float(np.min(step_ms)), 3), "ms_iteration_median": round(float(np.median(iter_ms)), 3),
                              "steps": a.steps, "device": name}), flush=True)
            if depth == 2:
                ms = C.c_float()
                _lib.check(lib.mpn_debug_bench_train_fc6(net._h, 20, C.byref(ms)), "mpn_debug_bench_train_fc6")
                k6, F = P["fc6_w"].shape[1], P["fc6_w"].shape[0]
                gb = 4 * (k6 * F * 4) / 1e9   # w read + w write + v read + v write (pad lanes of the packing: none at 25088 x 4096)
                print(json.dumps({"what": "fc6_wgrad_sgd_kernel", "ms": round(ms.value, 4), "gbytes_moved": round(gb, 3),
                                  "gbytes_per_s": round(gb / (ms.value * 1e-3), 1), "floor_ms_at_6.3TBps": round(gb / 6.3e3 * 1e3, 3), "device": name}), flush=True)
            if depth == 3:
                ms = C.c_float()
                _lib.check(lib.mpn_debug_bench_train_wgrad(net._h, 20, C.byref(ms)), "mpn_debug_bench_train_wgrad")
                gflop = 2 * 9 * 512 * 512 * 38 * 63 / 1e9
                floor_ms = gflop / 157.3e3 * 1e3
                print(json.dumps({"what": "conv3x3_wgrad_kernel", "layer": "conv5_3 512->512 38x63, one image", "ms": round(ms.value, 4), "gflop": round(gflop, 2),
                                  "tflops": round(gflop / ms.value, 1), "floor_ms_at_157.3TF": round(floor_ms, 4), "share_of_floor": round(floor_ms / ms.value, 3),
                                  "device": name}), flush=True)
            if depth == "trunk":
                ms, layer = C.c_float(), C.c_int()
                _lib.check(lib.mpn_debug_bench_train_poolbwd(net._h, 50, C.byref(ms), C.byref(layer)), "mpn_debug_bench_train_poolbwd")
                cout, h, w = P["conv_w"][layer.value].shape[0], H, W
                for l in range(layer.value):   # the layer's own map size: halved, rounding up, at every pool below it
                    if net._pool[l]:
                        h, w = (h + 1) // 2, (w + 1) // 2
                mb = 4 * cout * (2 * h * w + ((h + 1) // 2) * ((w + 1) // 2)) / 1e6
                floor_us = mb / 6.3
                print(json.dumps({"what": "maxpool2x2_backward_kernel", "layer": "conv layer %d, %d x %d x %d, one image" % (layer.value, cout, h, w),
                                  "us": round(ms.value * 1e3, 2), "mbytes_moved": round(mb, 1), "floor_us_at_6.3TBps": round(floor_us, 2),
                                  "share_of_floor": round(floor_us / (ms.value * 1e3), 3), "device": name}), flush=True)
            net.train_end()
        net.close()


if __name__ == "__main__":
    main()
