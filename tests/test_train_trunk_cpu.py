"""No GPU: tests/train_trunk_np.py — a training step through the trunk's pooling layers — checked against plain autograd, its first-maximum
routing on hand-written ties, and the public surface of MPN_TRAIN_TRUNK (include/mpn.h, the generated Lua declaration)."""
import os
import re
import subprocess
import sys

import numpy as np
import torch

import train_conv_np as TC
import train_np as T
import train_trunk_np as TT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANS = (3, 4, 6, 5, 6, 7, 8)            # six conv layers, pools after layers 1 and 3: the shape of the GPU tests' network
POOL = (0, 1, 0, 1, 0, 0)
STD, MEAN = [0.1, 0.1, 0.2, 0.2], [0.0] * 4


def _setup(seed=5, C=5, fc=16, sizes=((37, 45), (41, 35))):
    rng = np.random.default_rng(seed)
    k6 = CHANS[-1] * 49
    P = {"fc6_w": rng.standard_normal((fc, k6)) * (2.0 / k6) ** 0.5, "fc6_b": rng.standard_normal(fc) * 0.01,
         "fc7_w": rng.standard_normal((fc, fc)) * (2.0 / fc) ** 0.5, "fc7_b": rng.standard_normal(fc) * 0.01,
         "cls_w": rng.standard_normal((C, fc)) * 0.03, "cls_b": rng.standard_normal(C), "bbox_w": rng.standard_normal((4 * C, fc)) * 0.005,
         "bbox_b": rng.standard_normal(4 * C) * 0.1}
    conv = [(rng.standard_normal((CHANS[j + 1], CHANS[j], 3, 3)) * (2.0 / (9 * CHANS[j])) ** 0.5, rng.standard_normal(CHANS[j + 1]) * 0.01) for j in range(6)]
    images = []
    for (h, w), n in zip(sizes, (5, 3)):   # odd sizes: 37 -> 19 -> 10, 45 -> 23 -> 12; 41 -> 21 -> 11, 35 -> 18 -> 9
        im = rng.standard_normal((3, h, w))
        c = rng.uniform([6, 6], [w - 6, h - 6], (n, 2))
        wh = rng.uniform(8, 30, (n, 2))
        rois5 = np.concatenate([np.ones((n, 1)), c - wh / 2, c + wh / 2], 1).astype(np.float32)
        rois5[0, 1:] = [w + 30, h + 30, w + 40, h + 40]   # wholly outside the map: 49 empty bins
        images.append((im, rois5))
    rois = np.concatenate([im[1][:, 1:] for im in images])
    gt = rois + rng.normal(0, 0.4, (8, 4)).astype(np.float32)
    labels = rng.integers(0, C, 8)
    return P, conv, images, rois, gt, labels


def _forward(cw, cb, a, l0, l1):
    """layers l0 .. l1 - 1 of the trunk by plain torch: conv2d, relu, max_pool2d(ceil_mode=True)"""
    a = a[None]
    for l in range(l0, l1):
        a = torch.relu(torch.nn.functional.conv2d(a, cw[l], cb[l], padding=1))
        if POOL[l]:
            a = torch.nn.functional.max_pool2d(a, 2, 2, ceil_mode=True)
    return a[0]


def _plain_step(P, conv, images, rois, gt, labels, k, lr, momentum, wd):
    """the step with nothing handed in and no restatement of the pool: ordinary autograd, float64"""
    tr = TT.Trainer(P, conv, POOL, k, momentum, wd, mean=MEAN, std=STD, dtype=torch.float64, lr=lr)
    tr.opt.zero_grad()
    pooled = []
    for a0, rois5 in images:
        top = _forward(tr.cw, tr.cb, torch.as_tensor(a0), 6 - k, 6)
        _, H, W = top.shape
        for row in TC.roi_windows(rois5, H, W, 7, 7, 0.25):
            bins = [top[:, hs:he, ws:we].amax((1, 2)) if he > hs and we > ws else top.new_zeros(top.shape[0]) for hs, he, ws, we in row]
            pooled.append(torch.stack(bins, 1).reshape(-1))
    x = torch.stack(pooled)
    L_cls, L_box = tr.head(x, rois, gt, labels)
    (L_cls + L_box).backward()
    tr.opt.step()
    return tr.params(), x.detach().numpy()


def test_restatement_is_plain_autograd_for_every_trunk_depth():
    P, conv, images, rois, gt, labels = _setup()
    cw, cb = [torch.as_tensor(w) for w, _ in conv], [torch.as_tensor(b) for _, b in conv]
    for k in (1, 2, 3, 4, 5):
        sub = [(_forward(cw, cb, torch.as_tensor(im), 0, 6 - k).numpy(), r5) for im, r5 in images]
        want, x = _plain_step(P, conv, sub, rois, gt, labels, k, 0.1, 0.9, 5e-4)
        tr = TT.Trainer(P, conv, POOL, k, 0.9, 5e-4, mean=MEAN, std=STD, dtype=torch.float64)
        (l_cls, l_box), dx6 = tr.step(x, rois, gt, labels, [(a0, None, None, r5, None) for a0, r5 in sub], lr=0.1)
        got = tr.params()
        assert np.isfinite(l_cls) and np.isfinite(l_box) and dx6.shape == x.shape
        for name in T.TENSORS:
            assert np.allclose(got[name], want[name], rtol=1e-11, atol=1e-14), (k, name)
        for l in range(6):
            moved = not np.array_equal(got["conv_w"][l], conv[l][0])
            assert moved == (l >= 6 - k), (k, l)
            assert np.allclose(got["conv_w"][l], want["conv_w"][l], rtol=1e-11, atol=1e-14), (k, l)
            assert np.allclose(got["conv_b"][l], want["conv_b"][l], rtol=1e-11, atol=1e-14), (k, l)


def test_ties_route_to_the_first_maximum():
    x = np.array([[[2.0, 2.0], [1.0, 2.0]]])
    assert TT.first_max_route(x).tolist() == [[[0]]]
    g = np.array([[[5.0]]])
    assert TT.maxpool_backward_np(x, g, 0).tolist() == [[[5.0, 0.0], [0.0, 0.0]]]
    # a 3 x 5 map: ragged windows in the last row and column; ties between rows resolve to the upper cell, inside a row to the left one
    x = np.array([[[1.0, 3.0, 0.0, 0.0, -1.0],
                   [3.0, 3.0, 0.0, 0.0, -1.0],
                   [4.0, 4.0, -2.0, -2.0, np.nan]]])
    assert TT.first_max_route(x).tolist() == [[[1, 2, 4], [10, 12, -1]]]
    g = np.arange(1.0, 7.0).reshape(1, 2, 3)
    plain = TT.maxpool_backward_np(x, g, 0)
    want = np.zeros((3, 5))
    want[0, 1], want[0, 2], want[0, 4], want[2, 0], want[2, 2] = 1.0, 2.0, 3.0, 4.0, 5.0   # the NaN window routes nowhere
    assert np.array_equal(plain[0], want)
    masked = TT.maxpool_backward_np(x, g, 1)
    want[0, 2] = want[0, 4] = want[2, 2] = 0.0   # X <= 0: the all-zero window and the negative ones route nothing
    assert np.array_equal(masked[0], want)
    # torch's own pool makes the same choice where the maximum is unique, and the gather is its forward
    rng = np.random.default_rng(3)
    a = rng.standard_normal((4, 7, 9))
    r = TT.first_max_route(a)
    t = torch.as_tensor(a, dtype=torch.float64).requires_grad_(True)
    out = torch.nn.functional.max_pool2d(t[None], 2, 2, ceil_mode=True)[0]
    assert np.array_equal(TT.gather_pool2x2(t, r).detach().numpy(), out.detach().numpy())
    go = rng.standard_normal(out.shape)
    out.backward(torch.as_tensor(go))
    assert np.array_equal(t.grad.numpy(), TT.maxpool_backward_np(a, go, 0))


def test_given_routing_and_masks_are_used_not_recomputed():
    P, conv, images, rois, gt, labels = _setup(seed=9)
    cw, cb = [torch.as_tensor(w) for w, _ in conv], [torch.as_tensor(b) for _, b in conv]
    sub = [(_forward(cw, cb, torch.as_tensor(im), 0, 3).numpy(), r5) for im, r5 in images]   # trunk_layers 3 starts at the pooled layer 3

    def run(routes_of, masks_of):
        tr = TT.Trainer(P, conv, POOL, 3, 0.0, 0.0, mean=MEAN, std=STD, dtype=torch.float64)
        ims = []
        for a0, r5 in sub:
            h, w = a0.shape[1:]
            hp, wp = (h + 1) // 2, (w + 1) // 2
            shapes = [(CHANS[4], h, w), (CHANS[5], hp, wp), (CHANS[6], hp, wp)]
            ims.append((a0, masks_of(shapes), None, r5, routes_of(shapes)))
        tr.step(np.ones((8, CHANS[6] * 49)), rois, gt, labels, ims, lr=1.0)
        return tr.params()

    ones = lambda shapes: [np.ones(s, bool) for s in shapes]
    # every window of the pooled layer routed to cell (0, 0): only that pixel of its output gets a gradient, so the taps that read the
    # zero padding there (ky = 0 or kx = 0) keep their weights, whatever the activations say; the other four taps move
    corner = lambda shapes: [np.zeros((shapes[0][0], shapes[1][1], shapes[1][2]), np.int64), None, None]
    got = run(corner, ones)
    w0, w1 = conv[3][0], got["conv_w"][3]
    assert np.array_equal(w1[:, :, 0, :], w0[:, :, 0, :]) and np.array_equal(w1[:, :, :, 0], w0[:, :, :, 0])
    assert (w1[:, :, 1:, 1:] != w0[:, :, 1:, 1:]).any()
    own = run(lambda shapes: None, ones)
    assert (own["conv_w"][3][:, :, 0, :] != w0[:, :, 0, :]).any()
    # a mask that closes every ReLU of the pooled layer: no gradient reaches it, the two layers above still train
    closed = lambda shapes: [np.zeros(shapes[0], bool), np.ones(shapes[1], bool), np.ones(shapes[2], bool)]
    got = run(lambda shapes: None, closed)
    assert np.array_equal(got["conv_w"][3], conv[3][0]) and np.array_equal(got["conv_b"][3], conv[3][1])
    assert not np.array_equal(got["conv_b"][4], conv[4][1]) and not np.array_equal(got["conv_b"][5], conv[5][1])


def test_header_declares_the_trunk_depth_and_keeps_the_version():
    h = open(os.path.join(ROOT, "include", "mpn.h")).read()
    assert re.search(r"#define\s+MPN_VERSION\s+600\b", h)
    assert re.search(r"#define\s+MPN_TRAIN_TRUNK\(k\)\s+\(32 \+ \(k\)\)", h) and re.search(r"enum\s*\{\s*MPN_TRAIN_MAX_TRUNK\s*=\s*12\s*\}", h)
    assert re.search(r"#define\s+MPN_TRAIN_CONV\(k\)\s+\(MPN_TRAIN_FC6 \+ \(k\)\)", h) and re.search(r"enum\s*\{\s*MPN_TRAIN_MAX_CONV\s*=\s*7\s*\}", h)
    assert re.search(r"#define\s+MPN_TRAIN_MAX_IMAGES\s+8\b", h)
    assert re.search(r"\bint\s+mpn_maxpool2x2_ceil_backward\s*\(const float \*d_in, const float \*d_grad_out, int BC, int H, int W, int relu_mask, float \*d_grad_in,\s*void \*stream\)", h)


def test_lua_cdef_is_fresh_and_holds_the_new_prototype():
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_lua_cdef.py"), "--check"]) == 0
    cdef = open(os.path.join(ROOT, "multipathnet_amd", "lua", "mpn_cdef.lua")).read()
    assert "mpn_maxpool2x2_ceil_backward(" in cdef and "MPN_TRAIN_MAX_TRUNK = 12" in cdef
