"""No GPU: tests/train_conv_np.py's block stage checked against plain autograd, and the public surface of the conv-block training
(include/mpn.h, the generated Lua declaration)."""
import os
import re
import subprocess
import sys

import numpy as np
import torch

import train_conv_np as TC
import train_np as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _setup(seed=5, C=7, fc=24, chans=(6, 8, 5, 8), hw=(9, 13)):
    rng = np.random.default_rng(seed)
    k6 = chans[-1] * 49
    P = {"fc6_w": rng.standard_normal((fc, k6)) * (2.0 / k6) ** 0.5, "fc6_b": rng.standard_normal(fc) * 0.01,
         "fc7_w": rng.standard_normal((fc, fc)) * (2.0 / fc) ** 0.5, "fc7_b": rng.standard_normal(fc) * 0.01,
         "cls_w": rng.standard_normal((C, fc)) * 0.03, "cls_b": rng.standard_normal(C), "bbox_w": rng.standard_normal((4 * C, fc)) * 0.005,
         "bbox_b": rng.standard_normal(4 * C) * 0.1}
    conv = [(rng.standard_normal((chans[j + 1], chans[j], 3, 3)) * (2.0 / (9 * chans[j])) ** 0.5, rng.standard_normal(chans[j + 1]) * 0.01) for j in range(3)]
    images = []
    for i, n in enumerate((5, 3)):
        h, w = hw[0] + 2 * i, hw[1] - i
        a0 = np.abs(rng.standard_normal((chans[0], h, w)))
        c = rng.uniform([6, 6], [4 * w - 6, 4 * h - 6], (n, 2))
        wh = rng.uniform(8, 30, (n, 2))
        rois5 = np.concatenate([np.ones((n, 1)), c - wh / 2, c + wh / 2], 1).astype(np.float32)
        rois5[0, 1:] = [4 * w + 30, 4 * h + 30, 4 * w + 40, 4 * h + 40]   # wholly outside the map: 49 empty bins
        images.append((a0, rois5))
    B = 8
    rois = np.concatenate([im[1][:, 1:] for im in images])
    gt = rois + rng.normal(0, 0.4, (B, 4)).astype(np.float32)
    labels = rng.integers(0, C, B)
    return P, conv, images, rois, gt, labels, chans


def _plain_step(P, conv, images, rois, gt, labels, k, lr, momentum, wd):
    """the same step with nothing handed in: relu, and each bin the max over its window — ordinary autograd, float64"""
    tr = TC.Trainer(P, conv, 2 + k, momentum, wd, mean=[0.0] * 4, std=[0.1, 0.1, 0.2, 0.2], dtype=torch.float64, lr=lr)
    tr.opt.zero_grad()
    pooled = []
    for a0, rois5 in images:
        top = tr.block(a0)
        _, H, W = top.shape
        for row in TC.roi_windows(rois5, H, W, 7, 7, 0.25):
            bins = [top[:, hs:he, ws:we].amax((1, 2)) if he > hs and we > ws else top.new_zeros(top.shape[0]) for hs, he, ws, we in row]
            pooled.append(torch.stack(bins, 1).reshape(-1))
    x = torch.stack(pooled)
    L_cls, L_box = tr.head(x, rois, gt, labels)
    (L_cls + L_box).backward()
    tr.opt.step()
    return tr.params(), x.detach().numpy()


def test_block_stage_with_its_own_masks_and_argmax_is_plain_autograd():
    P, conv, images, rois, gt, labels, chans = _setup()
    for k in (1, 2, 3):
        sub = [(a0 if k == 3 else _forward_to(conv, a0, 3 - k), r5) for a0, r5 in images]
        want, x = _plain_step(P, conv, sub, rois, gt, labels, k, 0.1, 0.9, 5e-4)
        tr = TC.Trainer(P, conv, 2 + k, 0.9, 5e-4, mean=[0.0] * 4, std=[0.1, 0.1, 0.2, 0.2], dtype=torch.float64)
        (l_cls, l_box), dx6 = tr.step(x, rois, gt, labels, [(a0, None, None, r5) for a0, r5 in sub], lr=0.1)
        got = tr.params()
        assert np.isfinite(l_cls) and np.isfinite(l_box) and dx6.shape == x.shape
        for name in T.TENSORS:
            assert np.allclose(got[name], want[name], rtol=1e-12, atol=1e-14), name
        for j in range(3):
            moved = not np.array_equal(got["conv_w"][j], conv[j][0])
            assert moved == (j >= 3 - k), (k, j)
            assert np.allclose(got["conv_w"][j], want["conv_w"][j], rtol=1e-11, atol=1e-14), (k, j)
            assert np.allclose(got["conv_b"][j], want["conv_b"][j], rtol=1e-11, atol=1e-14), (k, j)
        # the head stage is train_np's: the same eight tensors from Sgd64
        ref = T.Sgd64(P, depth=2, momentum=0.9, weight_decay=5e-4, mean=[0.0] * 4, std=[0.1, 0.1, 0.2, 0.2])
        ref.step(x, rois, gt, labels, lr=0.1)
        for name in T.TENSORS:
            assert np.allclose(got[name], ref.P[name], rtol=1e-10, atol=1e-13), name


def _forward_to(conv, a0, n_layers):
    a = torch.as_tensor(a0)[None]
    for w, b in conv[:n_layers]:
        a = torch.relu(torch.nn.functional.conv2d(a, torch.as_tensor(w), torch.as_tensor(b), padding=1))
    return a[0].numpy()


def test_given_masks_and_argmax_are_used_not_recomputed():
    """with a mask that closes every ReLU of the last layer the block's gradients are exactly zero, whatever the activations say"""
    P, conv, images, rois, gt, labels, chans = _setup(seed=9)
    tr = TC.Trainer(P, conv, 5, 0.0, 0.0, mean=[0.0] * 4, std=[0.1, 0.1, 0.2, 0.2], dtype=torch.float64)
    ims = []
    for a0, r5 in images:
        h, w = a0.shape[1:]
        masks = [np.ones((chans[1], h, w), bool), np.ones((chans[2], h, w), bool), np.zeros((chans[3], h, w), bool)]
        ims.append((a0, masks, np.zeros((len(r5), chans[3], 49), np.int64), r5))
    tr.step(np.ones((8, chans[3] * 49)), rois, gt, labels, ims, lr=1.0)
    got = tr.params()
    assert all(np.array_equal(got["conv_w"][j], conv[j][0]) and np.array_equal(got["conv_b"][j], conv[j][1]) for j in range(3))
    assert not np.array_equal(got["fc6_w"], P["fc6_w"])


def test_roi_pool_backward_np_order():
    g = np.array([[[1e8, 1.0]], [[-1e8, 1.0]]], np.float32).reshape(2, 1, 2)
    am = np.zeros((2, 1, 2), np.int64)
    r5 = np.array([[1, 0, 0, 1, 1], [1, 0, 0, 1, 1]], np.float32)
    out = TC.roi_pool_backward_np(g, am, r5, 1, 1, 1, 1, np.float32)
    assert out[0, 0, 0, 0] == np.float32(np.float32(np.float32(np.float32(1e8) + np.float32(1)) + np.float32(-1e8)) + np.float32(1))   # ((1e8 + 1) - 1e8) + 1 = 1


def test_header_declares_the_new_functions_and_keeps_the_version():
    h = open(os.path.join(ROOT, "include", "mpn.h")).read()
    assert re.search(r"#define\s+MPN_VERSION\s+600\b", h)
    for fn in ("mpn_frcnn_get_trunk_weights", "mpn_roi_pool_backward", "mpn_conv3x3_backward"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, h), fn
    assert re.search(r"#define\s+MPN_TRAIN_CONV\(k\)\s+\(MPN_TRAIN_FC6 \+ \(k\)\)", h) and re.search(r"#define\s+MPN_TRAIN_MAX_IMAGES\s+8\b", h)


def test_lua_cdef_is_fresh():
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_lua_cdef.py"), "--check"]) == 0
    cdef = open(os.path.join(ROOT, "multipathnet_amd", "lua", "mpn_cdef.lua")).read()
    assert "mpn_conv3x3_backward(" in cdef and "mpn_roi_pool_backward(" in cdef and "mpn_frcnn_get_trunk_weights(" in cdef
