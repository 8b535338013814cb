"""Training the conv block above the trunk's last pooling layer on the device (depth MPN_TRAIN_CONV(k)) against
float64 (tests/train_conv_np.py), and the two module-level backward passes (mpn_roi_pool_backward, mpn_conv3x3_backward) on their own.

The float side never judges a forward pass and never decides anything: its head stage starts from the device's pooled operand
("train_pooled"), its block stage rebuilds the trained layers from the device's saved input map ("train_act.<i>.0") with the DEVICE's
ReLU masks ([train_act.<i>.<j> > 0]) and gathers at the DEVICE's argmax (nn.ROIPooling on train_act.<i>.<k>, whose output must equal
"train_pooled" bit for bit).  THE YARDSTICK RULE is tests/test_gpu_train.py's, unchanged: e = max(|r - r64| - u |w_new|, 0),
max e <= MARGIN max|r32 - r64| and rms e <= MARGIN rms|r32 - r64| with r32 the same program in torch.float32; every comparison prints
an `ACC` line.

Network: cfg [8, 16, P, 16, P, 32, 24, 40] — K = 3 trained layers 16 -> 32, 32 -> 24, 24 -> 40: multiples of 8 but not of 32 or 128, the
Winograd form present on all three —, 7 x 7 pooling (K6 = 1960), spatial scale 1/4, 96 x 160 maximum, max_rois 200; images 96 x 160
(24 x 40 map) and 81 x 135 (21 x 34 map: ceil pooling of odd sizes, ragged against the 8 x 32 conv tile).  Every handle first runs a
200-ROI detect and a 200-row depth-5 step at lr 0, so every buffer holds stale rows and stale maps.

MEASURED on MI355X (ACC lines of this file; largest max-ratio / rms-ratio over all cases of a test; yardstick = the same program in
torch.float32 on the CPU; conv3 / conv4 / conv5 = the block's layers 16 -> 32, 32 -> 24, 24 -> 40):
  gradient, depth 5 (6 cases): conv3_w 1.46 / 1.51  conv3_b 1.11 / 1.43  conv4_w 1.24 / 0.89  conv4_b 1.02 / 0.92  conv5_w 1.54 / 0.67
                               conv5_b 0.78 / 0.65  fc6_w 1.26 / 0.76  fc6_b 0.86 / 0.68  fc7_w 1.30 / 0.52  fc7_b 0.72 / 0.67
                               cls_w 1.08 / 0.83  cls_b 0.78 / 0.54  bbox_w 1.48 / 1.23  bbox_b 1.39 / 1.34  loss 0.69 / 0.72
  three steps, depths 3-5:     conv3_w 0.57 / 0.26  conv3_b 0.12 / 0.09  conv4_w 0.61 / 0.26  conv4_b 0.36 / 0.30  conv5_w 0.57 / 0.25
                               conv5_b 0.25 / 0.15  head tensors <= 0.88 / 0.47  losses 0.56 / 0.47
  mpn_conv3x3_backward (7):    grad_in 1.31 / 1.34  grad_w 1.80 / 1.55  grad_b 1.02 / 0.99
The largest is 1.80 (grad_w of 24 -> 40 at 21 x 34), inside the project's MARGIN = 2.0, which therefore holds for the conv tensors too."""
import numpy as np
import pytest
import torch

import train_conv_np as TC
import train_np as T

pytestmark = pytest.mark.gpu

CFG = [8, 16, "P", 16, "P", 32, 24, 40]
BLOCK = (3, 4, 5)            # indices of the K = 3 conv layers above the last pooling layer
CH = (16, 32, 24, 40)        # channels of the block's input map and of its layers' outputs
H, W, MAXR, K6 = 96, 160, 200, 40 * 49
SIZES = [(96, 160), (81, 135)]
HEADS = [(96, 7), (128, 4)]
STD, MEAN = [0.1, 0.1, 0.2, 0.2], [0.0, 0.0, 0.0, 0.0]
U = 2.0 ** -24
# The project's margin (tests/test_gpu_train.py).  The conv contractions run over ~10^3 pixels per image — longer chains than the head's
# B <= 128 rows; the weight gradient cuts them into 512-pixel segments, the bias gradient into 32 interleaved sums.
MARGIN = 2.0


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _params(fc, C, seed=557):
    from multipathnet_amd import models
    return models.synthetic_params(CFG, pooled=7, fc_dim=fc, n_classes=C, seed=seed, head_scale="trained")


def _np(P):
    out = {k: np.asarray(P[k].detach().cpu().numpy()) for k in T.TENSORS}
    out["conv_w"] = [w.detach().cpu().numpy() for w in P["conv_w"]]
    out["conv_b"] = [b.detach().cpu().numpy() for b in P["conv_b"]]
    return out


def _net(P, **kw):
    from multipathnet_amd import models
    return models.FastRCNN(P, cfg=CFG, pooled=7, spatial_scale=0.25, max_h=H, max_w=W, max_rois=MAXR, nms_thresh=0.3, **kw)


def _boxes(rng, n, h=H, w=W):
    c = rng.uniform([24, 24], [w - 24, h - 24], (n, 2))
    wh = rng.uniform(12, 44, (n, 2))
    return np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)


def _batch(seed, n, C, n_bg, size=(H, W)):
    """tests/test_gpu_train.py's recipe inside the image's own size"""
    rng = np.random.default_rng(seed)
    h, w = size
    im = rng.random((3, h, w), dtype=np.float32)
    rois = _boxes(rng, n, h, w)
    gt = rois + rng.normal(0, 0.4, (n, 4)).astype(np.float32)
    far = np.arange(n) % 3 == 0
    wv = (rois[:, 2] - rois[:, 0])[:, None]
    gt[far] = rois[far] + 0.5 * wv[far] * np.array([1, 0, 1, 0], np.float32)
    labels = rng.integers(1, C, n).astype(np.int32)
    labels[:n_bg] = 0
    gt[:n_bg] = 0
    return im, rois.astype(np.float32), gt.astype(np.float32), labels


def _add(net, dev, b):
    net.train_add(_t(b[0], dev), _t(b[1], dev), _t(b[2], dev), _t(b[3], dev))


def _weights(net):
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in net.head_weights().items()}
    tw = net.trunk_weights()
    out["conv_w"] = [w.cpu().numpy() for w in tw["conv_w"]]
    out["conv_b"] = [b.cpu().numpy() for b in tw["conv_b"]]
    return out


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def _all_bits(Wa, Wb):
    return all(_bits(Wa[k], Wb[k]) for k in T.TENSORS) and all(_bits(a, b) for k in ("conv_w", "conv_b") for a, b in zip(Wa[k], Wb[k]))


def _judge(tag, r, r64, r32, w_new=None, margin=MARGIN):
    r, r64, r32 = np.asarray(r, np.float64), np.asarray(r64, np.float64), np.asarray(r32, np.float64)
    e = np.abs(r - r64)
    if w_new is not None:
        e = np.maximum(e - U * np.abs(np.asarray(w_new, np.float64)), 0.0)
    y = np.abs(r32 - r64)
    em, er, ym, yr = float(e.max()), float(np.sqrt((e * e).mean())), float(y.max()), float(np.sqrt((y * y).mean()))
    print("ACC %-30s max e %.3g / torch-fp32 %.3g = %.2f   rms e %.3g / %.3g = %.2f" %
          (tag, em, ym, em / ym if ym else (0.0 if em == 0 else np.inf), er, yr, er / yr if yr else (0.0 if er == 0 else np.inf)))
    return em <= margin * ym and er <= margin * yr, (tag, em, ym, er, yr)


def _stale(net, dev, C):
    """a 200-ROI detect and a 200-row depth-5 step at lr 0: every operand buffer, saved map and argmax row holds values of a larger call"""
    rng = np.random.default_rng(99)
    im, bx = _t(rng.random((3, H, W), dtype=np.float32), dev), _t(_boxes(rng, MAXR), dev)
    s, b = net.detect(im, bx)
    W0 = _weights(net)
    net.train_begin(depth=5, momentum=0.0, weight_decay=0.0, bbox_weight=1.0)
    _add(net, dev, _batch(77, MAXR, C, 60))
    net.train_step(0.0)
    net.train_end()
    assert _all_bits(_weights(net), W0)
    return im, bx, s, b


def _device_images(net, dev, parts, k):
    """what the float side takes from the device after a step of the images `parts` at depth 2 + k: per image (a0, masks, argmax, rois5),
    and the pooled operand x [B, K6].  The argmax comes from nn.ROIPooling on the saved last map; its output must be "train_pooled"."""
    from multipathnet_amd import nn
    B = sum(len(p[3]) for p in parts)
    x = net.debug_tensor("train_pooled", (B, K6)).cpu().numpy()
    images, row = [], 0
    pool = nn.ROIPooling(7, 7, 0.25)
    for i, p in enumerate(parts):
        h, w = (p[0].shape[1] + 3) // 4, (p[0].shape[2] + 3) // 4
        acts = [net.debug_tensor("train_act.%d.%d" % (i, j), (CH[3 - k + j], h, w)) for j in range(k + 1)]
        n = len(p[3])
        rois5 = np.concatenate([np.ones((n, 1), np.float32), p[1]], 1)
        out = pool.forward((acts[k][None].contiguous(), _t(rois5, dev)))
        torch.cuda.synchronize()
        assert _bits(out.cpu().numpy().reshape(n, K6), x[row:row + n]), "image %d: nn.ROIPooling on train_act.%d.%d is not train_pooled" % (i, i, k)
        images.append((acts[0].cpu().numpy(), [(a > 0).cpu().numpy() for a in acts[1:]], pool.indices.cpu().numpy().reshape(n, 40, 49).astype(np.int64), rois5))
        row += n
    return x, images


def _join(parts):
    return np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts])


def _block_of(Wn):
    return [(Wn["conv_w"][l], Wn["conv_b"][l]) for l in BLOCK]


def _judge_all(tag, k, W_old, Wd, P64, P32, as_difference):
    """every head tensor and the k trained conv layers; as_difference: judge w_old - w_new (the gradient at lr 1) instead of w_new"""
    bad = []
    pairs = [(n, W_old[n], Wd[n], P64[n], P32[n]) for n in T.TENSORS]
    for j in range(3 - k, 3):
        l = BLOCK[j]
        pairs.append(("conv%d_w" % l, W_old["conv_w"][l], Wd["conv_w"][l], P64["conv_w"][j], P32["conv_w"][j]))
        pairs.append(("conv%d_b" % l, W_old["conv_b"][l], Wd["conv_b"][l], P64["conv_b"][j], P32["conv_b"][j]))
    for n, w0, wd, w64, w32 in pairs:
        assert np.isfinite(wd).all() and not _bits(wd, w0), "%s did not move" % n
        w0 = w0.astype(np.float64)
        ok, info = _judge("%s %s" % (tag, n), w0 - wd, w0 - w64, w0 - w32, w_new=wd) if as_difference else _judge("%s %s" % (tag, n), wd, w64, w32, w_new=wd)
        if not ok:
            bad.append(info)
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. depths and limits
# ---------------------------------------------------------------------------------------------------------------------------------
def test_depth_beyond_the_last_pool_is_refused(dev):
    from multipathnet_amd import MpnError
    fc, C = HEADS[1]
    net = _net(_params(fc, C))
    W0 = _weights(net)
    net.train_begin(depth=3, momentum=0.0, weight_decay=0.0)
    _add(net, dev, _batch(11, 40, C, 10))
    loss = net.train_step(0.1).cpu().numpy()
    net.train_end()
    W1 = _weights(net)
    assert np.isfinite(loss).all()
    assert not _bits(W1["conv_w"][5], W0["conv_w"][5]) and not _bits(W1["conv_b"][5], W0["conv_b"][5]) and np.isfinite(W1["conv_w"][5]).all()
    assert all(_bits(W1["conv_w"][l], W0["conv_w"][l]) and _bits(W1["conv_b"][l], W0["conv_b"][l]) for l in range(5))
    with pytest.raises(MpnError) as ei:
        net.train_begin(depth=6)
    assert "status -1" in str(ei.value) and "K = 3" in str(ei.value) and "pooling layer" in str(ei.value), str(ei.value)
    net.train_begin(depth=5)
    for i in range(8):
        _add(net, dev, _batch(20 + i, 10, C, 3, SIZES[i % 2]))
    with pytest.raises(MpnError) as ei:
        _add(net, dev, _batch(30, 10, C, 3))
    assert "status -1" in str(ei.value) and "MPN_TRAIN_MAX_IMAGES = 8" in str(ei.value), str(ei.value)
    net.train_step(1e-3)   # the eight pending images are still there, and the handle still works
    net.train_end()
    W2 = _weights(net)
    assert not _bits(W2["conv_w"][3], W1["conv_w"][3]) and all(np.isfinite(w).all() for w in W2["conv_w"])
    rng = np.random.default_rng(5)
    s, b = net.detect(_t(rng.random((3, H, W), dtype=np.float32), dev), _t(_boxes(rng, 50), dev))
    assert torch.isfinite(s).all() and torch.isfinite(b).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the gradient: momentum 0, wd 0, lr 1, depth 5, one step -> w_old - w_new is the gradient plus one rounding of the subtraction
# ---------------------------------------------------------------------------------------------------------------------------------
GRAD_BATCHES = {"B70_two_images": [(33, 9, 0), (37, 11, 1)], "B128_one_image": [(128, 40, 0)], "B1": [(1, 0, 1)]}


@pytest.mark.parametrize("head", HEADS, ids=["fc%d_C%d" % h for h in HEADS])
@pytest.mark.parametrize("case", list(GRAD_BATCHES))
def test_conv_gradient_against_float64(dev, head, case):
    fc, C = head
    P = _params(fc, C)
    P0 = _np(P)
    net = _net(P)
    _stale(net, dev, C)
    parts = [_batch(1000 + 17 * i + fc, n, C, n_bg, SIZES[sz]) for i, (n, n_bg, sz) in enumerate(GRAD_BATCHES[case])]
    if case == "B1":
        parts = [tuple(a[1:2] if j else a for j, a in enumerate(_batch(1234, 2, C, 0, SIZES[1])))]
    net.train_begin(depth=5, momentum=0.0, weight_decay=0.0, bbox_weight=1.0)
    for b in parts:
        _add(net, dev, b)
    loss = net.train_step(1.0).cpu().numpy()
    x, images = _device_images(net, dev, parts, 3)
    dx6 = net.debug_tensor("train_dx6", x.shape).cpu().numpy()
    Wd = _weights(net)
    net.train_end()
    rois, gt, labels = _join(parts)
    res = {}
    for dt in (torch.float64, torch.float32):
        tr = TC.Trainer(P0, _block_of(P0), 5, 0.0, 0.0, mean=MEAN, std=STD, dtype=dt)
        l, d = tr.step(x, rois, gt, labels, images, lr=1.0)
        res[dt] = (tr.params(), l, d * (x > 0))
    bad = _judge_all(case, 3, P0, Wd, res[torch.float64][0], res[torch.float32][0], as_difference=True)
    assert (dx6[x <= 0] == 0).all()   # the gradient at the pooled features carries the last conv layer's ReLU mask
    ok, info = _judge("%s dx6" % case, dx6, res[torch.float64][2], res[torch.float32][2])
    if not ok:
        bad.append(info)
    ok, info = _judge("%s loss" % case, loss, np.array(res[torch.float64][1]), np.array(res[torch.float32][1], np.float32), w_new=loss)
    if not ok:
        bad.append(info)
    for l in range(3):   # below the block: not one bit
        assert _bits(Wd["conv_w"][l], P0["conv_w"][l]) and _bits(Wd["conv_b"][l], P0["conv_b"][l]), l
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. three steps at lr 1e-3, momentum 0.9, wd 5e-4, a new two-image batch each step, depths 3, 4, 5; a second handle gives the same bits
# ---------------------------------------------------------------------------------------------------------------------------------
def _three_steps(net, dev, C, depth, lr=1e-3, seed0=2000):
    net.train_begin(depth=depth, momentum=0.9, weight_decay=5e-4, bbox_weight=1.0)
    steps, losses = [], []
    for i in range(3):
        parts = [_batch(seed0 + 2 * i, 40 - 9 * i, C, 8, SIZES[i % 2]), _batch(seed0 + 2 * i + 1, 21 + 4 * i, C, 5, SIZES[(i + 1) % 2])]
        for b in parts:
            _add(net, dev, b)
        losses.append(net.train_step(lr))
        x, images = _device_images(net, dev, parts, depth - 2)
        steps.append((x,) + _join(parts) + (images,))
    net.train_end()
    return steps, torch.stack(losses).cpu().numpy()


@pytest.mark.parametrize("depth", [3, 4, 5])
def test_three_steps_every_depth(dev, depth):
    fc, C = HEADS[0]
    P = _params(fc, C)
    P0 = _np(P)
    net = _net(P)
    _stale(net, dev, C)
    steps, losses = _three_steps(net, dev, C, depth)
    Wd = _weights(net)
    res = {}
    for dt in (torch.float64, torch.float32):
        tr = TC.Trainer(P0, _block_of(P0), depth, 0.9, 5e-4, mean=MEAN, std=STD, dtype=dt)
        ls = [tr.step(*st, lr=1e-3)[0] for st in steps]
        res[dt] = (tr.params(), ls)
    k = depth - 2
    bad = _judge_all("depth%d" % depth, k, P0, Wd, res[torch.float64][0], res[torch.float32][0], as_difference=False)
    ok, info = _judge("depth%d losses" % depth, losses, np.array(res[torch.float64][1]), np.array(res[torch.float32][1], np.float32), w_new=losses)
    if not ok:
        bad.append(info)
    for l in range(6 - k):   # outside the depth: not one bit
        assert _bits(Wd["conv_w"][l], P0["conv_w"][l]) and _bits(Wd["conv_b"][l], P0["conv_b"][l]), l
    assert not bad, bad
    net2 = _net(P)
    _stale(net2, dev, C)
    _, losses2 = _three_steps(net2, dev, C, depth)
    assert _bits(losses, losses2) and _all_bits(Wd, _weights(net2))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. lr 0: re-packing the Winograd form from the master pack is the identity
# ---------------------------------------------------------------------------------------------------------------------------------
def test_lr0_changes_no_bit(dev):
    fc, C = HEADS[0]
    net = _net(_params(fc, C))
    im, bx, s0, b0 = _stale(net, dev, C)
    W0 = _weights(net)
    net.train_begin(depth=5, momentum=0.0, weight_decay=0.0)
    _add(net, dev, _batch(4000, 50, C, 12))
    _add(net, dev, _batch(4001, 30, C, 7, SIZES[1]))
    net.train_step(0.0)
    net.train_end()
    assert _all_bits(_weights(net), W0)
    s1, b1 = net.detect(im, bx)
    assert _bits(s0.cpu().numpy(), s1.cpu().numpy()) and _bits(b0.cpu().numpy(), b1.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. every packed form agrees with the exported weights; a graph captured before training replays the trained weights
# ---------------------------------------------------------------------------------------------------------------------------------
def test_packed_forms_agree_with_exported_weights(dev):
    fc, C = HEADS[0]
    P = _params(fc, C)
    net = _net(P)
    net.set_graphs(True)
    im, bx, s0, b0 = _stale(net, dev, C)
    rng = np.random.default_rng(31)
    im_s, bx_s = _t(rng.random((3, 40, 56), dtype=np.float32), dev), _t(_boxes(rng, 20, 48, 60).clip(0, 39), dev)
    for _ in range(3):   # captured at the second sighting of these buffers, replayed at the third
        net.test_one_async(im, bx)
    torch.cuda.synchronize()
    cap0, rep0 = net.graph_stats()
    assert cap0 >= 1 and rep0 >= 1
    _three_steps(net, dev, C, 5, lr=1e-2)
    s1, b1 = net.detect(im, bx)
    s1s, b1s = [v.clone() for v in net.detect(im_s, bx_s)]
    runs = []
    for _ in range(3):
        d, n = net.test_one_async(im, bx)
        torch.cuda.synchronize()
        runs.append((d.cpu().numpy().copy(), int(n.item())))
    cap1, rep1 = net.graph_stats()
    assert rep1 > rep0, "no graph was replayed after training"
    Pn = dict(P)
    Pn.update({k: v.cpu() for k, v in net.head_weights().items()})
    Pn.update({k: [v.cpu() for v in vs] for k, vs in net.trunk_weights().items()})
    fresh = _net(Pn)
    s2, b2 = fresh.detect(im, bx)
    assert _bits(s1.cpu().numpy(), s2.cpu().numpy()) and _bits(b1.cpu().numpy(), b2.cpu().numpy())
    s2s, b2s = fresh.detect(im_s, bx_s)
    assert _bits(s1s.cpu().numpy(), s2s.cpu().numpy()) and _bits(b1s.cpu().numpy(), b2s.cpu().numpy())
    d2, n2 = fresh.test_one_async(im, bx)
    torch.cuda.synchronize()
    n2 = int(n2.item())
    assert n2 > 0
    for d, n in runs:
        assert n == n2 and _bits(d[:min(n, d.shape[0])], d2.cpu().numpy()[:min(n2, d.shape[0])])
    assert _all_bits(_weights(net), _weights(fresh))   # unpack -> create -> unpack
    assert not _bits(s0.cpu().numpy(), s1.cpu().numpy()), "training did not change what detect computes"


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. mpn_roi_pool_backward is the ordered sum
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 40])
@pytest.mark.parametrize("n_rows", [1, 37])
@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (21, 34)], ids=["1x1", "5x7", "21x34"])
def test_roi_pool_backward_is_the_ordered_sum(dev, hw, n_rows, C):
    from multipathnet_amd import nn
    h, w = hw
    rng = np.random.default_rng(600 + h + n_rows + C)
    feat = rng.standard_normal((2, C, h, w)).astype(np.float32)
    c = rng.uniform([-8, -8], [4 * w + 8, 4 * h + 8], (n_rows, 2))           # some boxes stick out of the map: empty bins
    wh = rng.uniform(4, max(8.0, 3.0 * max(h, w)), (n_rows, 2))
    rois = np.concatenate([rng.integers(1, 3, (n_rows, 1)), c - wh / 2, c + wh / 2], 1).astype(np.float32)
    if n_rows > 4:
        rois[5], rois[9] = rois[2], rois[2]                                  # duplicated boxes: several rows add into the same cells
        rois[11] = [1, 4 * w + 40, 4 * h + 40, 4 * w + 60, 4 * h + 60]       # wholly outside
    pool = nn.ROIPooling(7, 7, 0.25)
    pool.forward((_t(feat, dev), _t(rois, dev)))
    am = pool.indices.cpu().numpy()
    g = rng.standard_normal((n_rows, C, 7, 7)).astype(np.float32)
    got = pool.updateGradInput((_t(feat, dev), _t(rois, dev)), _t(g, dev))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want = TC.roi_pool_backward_np(g, am, rois, 2, C, h, w, np.float32)
    assert (am < 0).any() or hw == (21, 34) or n_rows == 1
    assert _bits(got, want)
    r64 = TC.roi_pool_backward_np(g, am, rois, 2, C, h, w, np.float64)
    cnt = TC.roi_pool_backward_np(np.ones_like(g), am, rois, 2, C, h, w, np.float64)
    mag = TC.roi_pool_backward_np(np.abs(g), am, rois, 2, C, h, w, np.float64)
    assert (np.abs(got - r64) <= cnt * U * mag).all()   # fp32 summation error: at most one rounding of the running sum per term


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. mpn_conv3x3_backward against torch float64 autograd, torch float32 the yardstick
# ---------------------------------------------------------------------------------------------------------------------------------
CONV_SHAPES = [(8, 8, 1, 1, 1), (12, 20, 6, 5, 1), (16, 24, 5, 7, 1), (24, 40, 21, 34, 1), (32, 136, 9, 33, 1), (40, 16, 24, 40, 1), (32, 32, 38, 63, 2)]


def _torch_conv_backward(x, w, g, dtype):
    xt, wt = torch.as_tensor(x).to(dtype).requires_grad_(True), torch.as_tensor(w).to(dtype).requires_grad_(True)
    bt = torch.zeros(w.shape[0], dtype=dtype, requires_grad=True)
    torch.nn.functional.conv2d(xt, wt, bt, padding=1).backward(torch.as_tensor(g).to(dtype))
    return xt.grad.numpy(), wt.grad.numpy(), bt.grad.numpy()


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=["%dto%d_%dx%d_B%d" % s for s in CONV_SHAPES])
def test_conv3x3_backward_against_float64(dev, shape):
    from multipathnet_amd import nn
    Cin, Cout, h, w, B = shape
    rng = np.random.default_rng(700 + Cin + Cout + h)
    x = rng.standard_normal((B, Cin, h, w)).astype(np.float32)
    wt = (rng.standard_normal((Cout, Cin, 3, 3)) * (2.0 / (Cin * 9)) ** 0.5).astype(np.float32)
    g = rng.standard_normal((B, Cout, h, w)).astype(np.float32)
    m = nn.SpatialConvolution(Cin, Cout)
    m.weight, m.bias = _t(wt, dev), _t(np.zeros(Cout, np.float32), dev)
    dx, dg = _t(x, dev), _t(g, dev)
    run = lambda a, b, c: [None if v is None else v.cpu().numpy() for v in m._backward(dx, dg, a, b, c)]
    full = run(True, True, True)
    r64, r32 = _torch_conv_backward(x, wt, g, torch.float64), _torch_conv_backward(x, wt, g, torch.float32)
    bad = []
    for name, r, a, b in zip(("grad_in", "grad_w", "grad_b"), full, r64, r32):
        assert np.isfinite(r).all()
        ok, info = _judge("%dto%d %dx%d B%d %s" % (Cin, Cout, h, w, B, name), r, a, b)
        if not ok:
            bad.append(info)
    # each output alone and in pairs: the same bits
    for sel in [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1)]:
        out = run(*[bool(v) for v in sel])
        for v, f, on in zip(out, full, sel):
            assert (v is None) == (not on) and (v is None or _bits(v, f)), sel
    # a workspace full of garbage (every halo and pad lane NaN) before the call, and a second run: the same bits
    m._bws.fill_(0xFF)
    again = run(True, True, True)
    assert all(_bits(a, f) for a, f in zip(again, full))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. state: a detect between train_add and train_step disturbs nothing; train_end frees everything; a second cycle works
# ---------------------------------------------------------------------------------------------------------------------------------
def test_detect_between_add_and_step_and_a_second_cycle(dev):
    fc, C = HEADS[1]
    P = _params(fc, C)
    parts = [_batch(8000, 40, C, 10, SIZES[1]), _batch(8001, 30, C, 8)]

    def cycle(net, with_detect):
        net.train_begin(depth=5, momentum=0.9, weight_decay=5e-4)
        _add(net, dev, parts[0])
        if with_detect:
            rng = np.random.default_rng(3)
            net.detect(_t(rng.random((3, 70, 90), dtype=np.float32), dev), _t(_boxes(rng, 150, 70, 90).clip(0, 69), dev))
        _add(net, dev, parts[1])
        if with_detect:
            rng = np.random.default_rng(4)
            net.detect(_t(rng.random((3, H, W), dtype=np.float32), dev), _t(_boxes(rng, MAXR), dev))
        loss = net.train_step(1e-2).cpu().numpy()
        net.train_end()
        return loss

    a, b = _net(P), _net(P)
    _stale(a, dev, C)
    _stale(b, dev, C)
    la, lb = cycle(a, False), cycle(b, True)
    assert _bits(la, lb) and _all_bits(_weights(a), _weights(b))
    from multipathnet_amd import MpnError
    with pytest.raises(MpnError):
        b.train_end()
    with pytest.raises(MpnError) as ei:
        b.debug_tensor("train_act.0.0", (16, 24, 40))
    assert "status -5" in str(ei.value)
    la2, lb2 = cycle(a, True), cycle(b, False)   # a second begin / end cycle on both
    assert _bits(la2, lb2) and _all_bits(_weights(a), _weights(b)) and not _bits(la, la2)
