"""Digests of what the training driver computes (csrc/train_driver.hip), to compare two builds bit for bit: a
changed launch order or a dropped launch that stays inside the float64 tests' tolerances still changes a digest.  Small networks, a few
seconds per scenario; every scenario is three SGD steps (momentum 0.9, weight decay 5e-4, lr 1e-3) of two images with 33 and 37 rows.

Plain handle (the six-layer VGG configuration of tests/test_gpu_train_trunk.py, 96 x 160 and 81 x 135 images): depth 0, 1, 2,
MPN_TRAIN_CONV(2), MPN_TRAIN_TRUNK(3) (the smallest k that crosses a pooling layer), depth 2 with dropout 0.5, depth 2 with K = 2
classifiers and train_set_head(1) on the middle step, depth 2 through train_add_sampled (the second image flipped) with
train_state() -> train_end -> train_begin -> train_load_state() between steps two and three.  After every step: head_weights(),
trunk_weights(), train_state().
MultiPathNet handle (network A of tests/test_gpu_train_towers.py, 150 x 250, the five towers, K = 2): plain, dropout 0.5 with
tower_train_set_head(1) on the middle step, through tower_train_add_sampled with one flipped image.  After every step: tower_weights()
and the debug tensors tower_train_cat and tower_train_g_cls.

One line per tensor: scenario, step, name, SHA-256 of its fp32 bytes; one line per step with the two loss values (hex floats).
--package-root DIR imports multipathnet_amd from another tree (a build of another commit); the outputs of two runs are compared as text.

    python tools/train_digest.py [--package-root DIR] [--time-limit 300] > digest.txt
"""
import argparse
import hashlib
import os
import signal
import sys

import numpy as np

VGG_CFG = [8, 16, "P", 16, 24, "P", 32, 40]
VGG_SIZES = [(96, 160), (81, 135)]
MPN_CFG = [8, 16, "P", 16, 24, "P", 32, 32, "P", 64, "P", 64]
MPN_SIZE = (150, 250)
ROWS = (33, 37)
BG = (9, 11)
STEPS, LR = 3, 1e-3


def rows_case(seed, n, n_classes, n_bg, size):
    """one image and its n rows: the first n_bg background, every third foreground row regressing to a far GT box"""
    rng = np.random.default_rng(seed)
    h, w = size
    im = rng.random((3, h, w), dtype=np.float32)
    c = rng.uniform([24, 24], [w - 24, h - 24], (n, 2))
    wh = rng.uniform(12, 44, (n, 2))
    rois = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    gt = rois + rng.normal(0, 0.4, (n, 4)).astype(np.float32)
    far = np.arange(n) % 3 == 0
    gt[far] = rois[far] + 0.5 * (rois[:, 2] - rois[:, 0])[far, None] * np.array([1, 0, 1, 0], np.float32)
    labels = rng.integers(1, n_classes, n).astype(np.int32)
    labels[:n_bg] = 0
    gt[:n_bg] = 0
    return im, rois, gt.astype(np.float32), labels


def proposals_case(seed, n_classes, size, n=60):
    """one image with 3 GT boxes, n proposals (jittered and shifted copies of them, one inside the crowd strip) and one crowd strip"""
    rng = np.random.default_rng(seed)
    h, w = size
    im = rng.random((3, h, w), dtype=np.float32)
    gt = np.zeros((3, 4), np.float32)
    for j in range(3):
        x1, y1 = rng.integers(8, w - 70), rng.integers(8, h - 50)
        gt[j] = [x1, y1, x1 + rng.integers(24, 56), y1 + rng.integers(20, 40)]
    gl = rng.integers(1, n_classes, 3).astype(np.int32)
    crowd = np.array([[w - 9, 0, w - 2, 2 * h]], np.float32)
    prop = np.zeros((n, 4), np.float32)
    prop[0] = [w - 9, 1, w - 2, h - 1]
    for i in range(1, n):
        b = gt[i % 3]
        d = rng.uniform(-2, 2, 4) if i % 2 else 0.45 * (b[2] - b[0]) * np.array([1, 0, 1, 0]) + rng.uniform(-1, 1, 4)
        prop[i] = np.clip(b + d.astype(np.float32), 1, [w, h, w, h])
    return im, prop, gt, gl, crowd


def emit(scn, step, name, t):
    a = np.ascontiguousarray(t.detach().cpu().numpy().astype("<f4", copy=False))
    print("%s step%d %s %s %s" % (scn, step, name, "x".join(map(str, a.shape)), hashlib.sha256(a.tobytes()).hexdigest()), flush=True)


def emit_tree(scn, step, prefix, v):
    """every tensor under a dict / list of the weight and state getters; integers (the step counter) as text, None as 'none'"""
    import torch
    if isinstance(v, dict):
        for k in sorted(v):
            emit_tree(scn, step, "%s.%s" % (prefix, k), v[k])
    elif isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            emit_tree(scn, step, "%s.%d" % (prefix, i), x)
    elif isinstance(v, torch.Tensor):
        emit(scn, step, prefix, v.float())
    elif v is None or isinstance(v, (int, str, bool)):
        print("%s step%d %s = %s" % (scn, step, prefix, "none" if v is None else v), flush=True)


def emit_loss(scn, step, loss):
    import torch
    torch.cuda.synchronize()
    a = loss.cpu().numpy()
    print("%s step%d loss %s %s" % (scn, step, float(a[0]).hex(), float(a[1]).hex()), flush=True)


def add_images(net, scn, step, sampled, tower, n_classes, sizes, dev):
    import torch
    from multipathnet_amd import train
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for j in range(2):
        seed = 3000 + 10 * step + j
        if sampled:
            im, prop, gt, gl, crowd = proposals_case(seed, n_classes, sizes[j])
            smp = train.DeviceRoiSampler(ROWS[j], 0.25, 0.5, (0.1, 0.5), seed=777)
            add = net.tower_train_add_sampled if tower else net.train_add_sampled
            counts = add(t(im), prop, gt, gl, smp, draw=2 * step + j, crowd_boxes=crowd, flip=(j == 1))
            print("%s step%d image%d counts %d %d" % (scn, step, j, counts[0], counts[1]), flush=True)
        else:
            b = rows_case(seed, ROWS[j], n_classes, BG[j], sizes[j])
            (net.tower_train_add if tower else net.train_add)(*[t(x) for x in b])


def plain_scenario(scn, dev, begin, K=1, sampled=False):
    import torch
    from multipathnet_amd import models
    C_ = 7
    P = models.synthetic_params(VGG_CFG, pooled=7, fc_dim=96, n_classes=C_, seed=557, head_scale="trained")
    if K > 1:
        P = models.integral_params(P, K)
    net = models.FastRCNN(P, cfg=VGG_CFG, pooled=7, spatial_scale=0.25, max_h=96, max_w=160, max_rois=200, nms_thresh=0.3)
    begin = dict(begin, momentum=0.9, weight_decay=5e-4)
    net.train_begin(**begin)
    for step in range(STEPS):
        if K > 1:
            net.train_set_head(1 if step == 1 else 0)
        if sampled and step == 2:   # a resumed run: the optimiser's state through its getter and setter
            S = net.train_state()
            net.train_end()
            net.train_begin(**begin)
            net.train_load_state(S)
        add_images(net, scn, step, sampled, False, C_, VGG_SIZES, dev)
        emit_loss(scn, step, net.train_step(LR))
        emit_tree(scn, step, "head_weights", net.head_weights())
        emit_tree(scn, step, "trunk_weights", net.trunk_weights())
        emit_tree(scn, step, "train_state", net.train_state())
    net.train_end()
    net.close()
    torch.cuda.synchronize()


def tower_scenario(scn, dev, dropout=0.0, heads=False, sampled=False):
    import torch
    from multipathnet_amd import models
    C_, K, F = 5, 2, 128
    P = models.synthetic_mpnet_params(MPN_CFG, pooled=7, fc_dim=F, n_classes=C_, n_integral=K, seed=557)
    net = models.MultiPathNet(P, cfg=MPN_CFG, pooled=7, spatial_scale=1.0 / 16, max_h=MPN_SIZE[0], max_w=MPN_SIZE[1], max_rois=200, nms_thresh=0.3)
    T = len(P["towers"])
    net.tower_train_begin(momentum=0.9, weight_decay=5e-4, dropout=dropout)
    for step in range(STEPS):
        if heads:
            net.tower_train_set_head(1 if step == 1 else 0)
        add_images(net, scn, step, sampled, True, C_, [MPN_SIZE, MPN_SIZE], dev)
        emit_loss(scn, step, net.tower_train_step(LR))
        emit_tree(scn, step, "tower_weights", net.tower_weights())
        emit(scn, step, "tower_train_cat", net.debug_tensor("tower_train_cat", (-1, T * F)))
        emit(scn, step, "tower_train_g_cls", net.debug_tensor("tower_train_g_cls", (-1, K * C_)))
    net.tower_train_end()
    net.close()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the tree multipathnet_amd is imported from (default: this one)")
    ap.add_argument("--time-limit", type=int, default=300, help="seconds after which the whole run is given up")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    signal.alarm(a.time_limit)   # (the default action ends the process)
    import torch
    assert torch.cuda.is_available(), "train_digest needs a HIP device"
    dev = torch.device("cuda")
    plain_scenario("plain_depth0", dev, dict(depth=0))
    plain_scenario("plain_depth1", dev, dict(depth=1))
    plain_scenario("plain_depth2", dev, dict(depth=2))
    plain_scenario("plain_conv2", dev, dict(depth=4))            # MPN_TRAIN_CONV(2)
    plain_scenario("plain_trunk3", dev, dict(trunk_layers=3))    # MPN_TRAIN_TRUNK(3): conv layers 3, 4, 5 — through the pool behind layer 3
    plain_scenario("plain_dropout", dev, dict(depth=2, dropout=0.5))
    plain_scenario("plain_integral2", dev, dict(depth=2), K=2)
    plain_scenario("plain_sampled_resumed", dev, dict(depth=2), sampled=True)
    tower_scenario("towers", dev)
    tower_scenario("towers_dropout_heads", dev, dropout=0.5, heads=True)
    tower_scenario("towers_sampled", dev, sampled=True)
    print("done", flush=True)


if __name__ == "__main__":
    main()
