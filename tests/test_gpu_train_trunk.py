"""Training the trunk through its pooling layers on the device (depth MPN_TRAIN_TRUNK(k), FastRCNN.train_begin(trunk_layers=k); DESIGN.md
section 13.5) against float64 (tests/train_trunk_np.py), and mpn_maxpool2x2_ceil_backward on its own against a numpy restatement, bit for bit.

The float side never judges a forward pass and never decides anything (tests/test_gpu_train_conv.py's rule, extended to the pools): its
head stage starts from the device's pooled operand ("train_pooled"); its trunk stage rebuilds the trained layers from the device's saved
input map ("train_act.<i>.0") with the DEVICE's ReLU masks ([train_act.<i>.<j> > 0], j >= 1: the maps before the pools), pools by a gather
at the DEVICE's routing — derived in numpy from those same pre-pool maps by the first-maximum rule — and ROI-pools at the DEVICE's argmax
(nn.ROIPooling on train_act.<i>.<k>, whose output must equal "train_pooled" bit for bit).  No case is excluded.  THE YARDSTICK RULE is
tests/test_gpu_train.py's, unchanged: e = max(|r - r64| - u |w_new|, 0), max e <= MARGIN max|r32 - r64| and rms e <= MARGIN rms|r32 - r64|
with r32 the same program in torch.float32 and MARGIN = 2.0; every comparison prints an `ACC` line.

Network: cfg [8, 16, P, 16, 24, P, 32, 40] — six conv layers, pools after layers 1 and 3, K = 2 —, 7 x 7 pooling (K6 = 1960), spatial scale
1/4, 96 x 160 maximum, max_rois 200; images 96 x 160 (maps 96 x 160 / 48 x 80 / 24 x 40) and 81 x 135 (81 x 135 / 41 x 68 / 21 x 34: ceil
pooling of odd sizes).  trunk_layers 3 starts at a pooled layer, 4 has a pooled layer in the middle, 5 crosses both pools; at 96 x 160 the
weight gradient of layer 1 sums 30 segments of 512 pixels (in groups of 8).  Every handle first runs a 200-ROI detect and a 200-row
trunk_layers-5 step at lr 0, so every buffer holds stale rows and stale maps.

MEASURED on MI355X (ACC lines of this file; largest max-ratio / rms-ratio over all cases of a test; yardstick = the same program in
torch.float32 on the CPU; conv1 .. conv5 = the trunk's layers 8 -> 16 (pooled), 16 -> 16, 16 -> 24 (pooled), 24 -> 32, 32 -> 40):
  gradient, trunk_layers 5 (6 cases): conv1_w 0.60 / 0.53  conv1_b 1.06 / 1.04  conv2_w 1.23 / 0.94  conv2_b 0.76 / 0.95  conv3_w 0.91 / 0.68
                                      conv3_b 1.00 / 0.97  conv4_w 1.13 / 0.79  conv4_b 0.59 / 0.61  conv5_w 1.24 / 0.67  conv5_b 0.71 / 0.56
                                      fc6_w 0.87 / 0.75  fc6_b 0.85 / 0.69  fc7_w 0.89 / 0.61  fc7_b 0.71 / 0.50  cls_w 1.17 / 0.81
                                      cls_b 0.45 / 0.26  bbox_w 1.02 / 0.95  bbox_b 0.98 / 0.97  dx6 1.05 / 0.85  loss 1.01 / 0.97
  three steps, trunk_layers 3-5:      conv tensors <= 0.61 / 0.27  head tensors <= 0.69 / 0.48  losses 1.50 / 1.47
The largest is 1.50 (the three losses at trunk_layers 4), inside the project's MARGIN = 2.0; the largest conv tensor is 1.24."""
import numpy as np
import pytest
import torch

import train_np as T
import train_trunk_np as TT

pytestmark = pytest.mark.gpu

CFG = [8, 16, "P", 16, 24, "P", 32, 40]
COUT = (8, 16, 16, 24, 32, 40)     # output channels of the six conv layers
POOL = (0, 1, 0, 1, 0, 0)          # pool_after
NL = 6
H, W, MAXR, K6 = 96, 160, 200, 40 * 49
SIZES = [(96, 160), (81, 135)]
HEADS = [(96, 7), (128, 4)]
STD, MEAN = [0.1, 0.1, 0.2, 0.2], [0.0, 0.0, 0.0, 0.0]
U = 2.0 ** -24
MARGIN = 2.0                       # the project's margin (tests/test_gpu_train.py, tests/test_gpu_train_conv.py)


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
    """a 200-ROI detect and a 200-row trunk_layers-5 step at lr 0: every operand buffer, saved map and argmax row holds values of a larger call"""
    rng = np.random.default_rng(99)
    im, bx = _t(rng.random((3, H, W), dtype=np.float32), dev), _t(_boxes(rng, MAXR), dev)
    s, b = [v.clone() for v in net.detect(im, bx)]
    W0 = _weights(net)
    net.train_begin(trunk_layers=5, momentum=0.0, weight_decay=0.0, bbox_weight=1.0)
    _add(net, dev, _batch(77, MAXR, C, 60))
    net.train_step(0.0)
    net.train_end()
    assert _all_bits(_weights(net), W0)
    return im, bx, s, b


def _map_shapes(size, k):
    """[C, h, w] of the saved maps j = 0..k of an image of `size` at trunk_layers k"""
    first = NL - k
    hw = [size]
    for l in range(NL):   # hw[l]: layer l's input and output size
        hw.append(((hw[l][0] + 1) // 2, (hw[l][1] + 1) // 2) if POOL[l] else hw[l])
    return [(COUT[first - 1],) + hw[first]] + [(COUT[first + j - 1],) + hw[first + j - 1] for j in range(1, k + 1)]


def _device_images(net, dev, parts, k):
    """what the float side takes from the device after a step of the images `parts` at trunk_layers k: per image (a0, masks, argmax, rois5,
    routes), and the pooled operand x [B, K6].  The argmax comes from nn.ROIPooling on the saved last map; its output must be "train_pooled"."""
    from multipathnet_amd import nn
    B = sum(len(p[3]) for p in parts)
    x = net.debug_tensor("train_pooled", (B, K6)).cpu().numpy()
    images, row = [], 0
    pool = nn.ROIPooling(7, 7, 0.25)
    first = NL - k
    for i, p in enumerate(parts):
        shapes = _map_shapes(p[0].shape[1:], k)
        acts = [net.debug_tensor("train_act.%d.%d" % (i, j), shapes[j]).clone() for j in range(k + 1)]
        n = len(p[3])
        rois5 = np.concatenate([np.ones((n, 1), np.float32), p[1]], 1)
        out = pool.forward((acts[k][None].contiguous(), _t(rois5, dev)))
        torch.cuda.synchronize()
        assert _bits(out.cpu().numpy().reshape(n, K6), x[row:row + n]), "image %d: nn.ROIPooling on train_act.%d.%d is not train_pooled" % (i, i, k)
        maps = [a.cpu().numpy() for a in acts]
        routes = [TT.first_max_route(maps[j]) if POOL[first + j - 1] else None for j in range(1, k + 1)]
        images.append((maps[0], [m > 0 for m in maps[1:]], pool.indices.cpu().numpy().reshape(n, 40, 49).astype(np.int64), rois5, routes))
        row += n
    return x, images


def _join(parts):
    return np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts])


def _trunk_of(Wn):
    return [(Wn["conv_w"][l], Wn["conv_b"][l]) for l in range(NL)]


def _judge_all(tag, k, W_old, Wd, P64, P32, as_difference):
    """every head tensor and the k trained conv layers; as_difference: judge w_old - w_new (the gradient at lr 1) instead of w_new"""
    bad = []
    pairs = [(n, W_old[n], Wd[n], P64[n], P32[n]) for n in T.TENSORS]
    for l in range(NL - k, NL):
        pairs.append(("conv%d_w" % l, W_old["conv_w"][l], Wd["conv_w"][l], P64["conv_w"][l], P32["conv_w"][l]))
        pairs.append(("conv%d_b" % l, W_old["conv_b"][l], Wd["conv_b"][l], P64["conv_b"][l], P32["conv_b"][l]))
    for n, w0, wd, w64, w32 in pairs:
        assert np.isfinite(wd).all() and not _bits(wd, w0), "%s did not move" % n
        w0 = w0.astype(np.float64)
        ok, info = _judge("%s %s" % (tag, n), w0 - wd, w0 - w64, w0 - w32, w_new=wd) if as_difference else _judge("%s %s" % (tag, n), wd, w64, w32, w_new=wd)
        if not ok:
            bad.append(info)
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. mpn_maxpool2x2_ceil_backward is the routing of the contract, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 1, 1), (3, 1, 5), (8, 2, 2), (5, 7, 9), (16, 21, 34), (24, 81, 135)]


@pytest.mark.parametrize("relu_mask", [0, 1])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=["%dx%dx%d" % s for s in POOL_SHAPES])
def test_maxpool_backward_is_the_routing(dev, shape, relu_mask):
    from multipathnet_amd import _lib, nn
    BC, h, w = shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    rng = np.random.default_rng(900 + BC + h + w)
    x = (rng.integers(-4, 5, (BC, h, w)) * 0.25).astype(np.float32)       # multiples of 0.25 in [-1, 1]: ties and non-positive windows
    g = rng.standard_normal((BC, ho, wo)).astype(np.float32)
    g[g == 0] = 1.0
    want = TT.maxpool_backward_np(x, g, relu_mask)
    if BC * ho * wo >= 100:   # (the three smallest shapes have too few windows to promise either)
        full = x[:, :h - h % 2, :w - w % 2].reshape(BC, h // 2, 2, w // 2, 2).transpose(0, 1, 3, 2, 4).reshape(BC, h // 2, w // 2, 4)
        mx = full.max(-1)
        assert ((full == mx[..., None]).sum(-1) > 1).any(), "no tie among the windows' maxima"
        assert (mx <= 0).any() and (mx > 0).any(), "no non-positive window"
    dx, dg = _t(x, dev), _t(g, dev)
    got = torch.full((BC, h, w), float("nan"), dtype=torch.float32, device=dev)   # poisoned: every element must be written
    rc = _lib.load().mpn_maxpool2x2_ceil_backward(nn._f(dx), nn._f(dg), BC, h, w, relu_mask, nn._f(got), nn._stream())
    torch.cuda.synchronize()
    assert rc == 0
    got = got.cpu().numpy()
    assert not np.isnan(got).any(), "an element of the gradient was not written"
    assert _bits(got, want)
    assert (np.count_nonzero(got.reshape(BC, -1), axis=1) <= ho * wo).all()
    if not relu_mask:
        m = nn.SpatialMaxPooling()
        gi = m.updateGradInput(dx, dg)
        torch.cuda.synchronize()
        assert _bits(gi.cpu().numpy(), want)
        gi4 = m.updateGradInput(dx[None], dg[None])    # leading dimensions fold into B * C
        torch.cuda.synchronize()
        assert gi4.shape == (1, BC, h, w) and _bits(gi4.cpu().numpy()[0], want)
        # against torch's own pool where the maximum of every window is unique (ties: torch also takes the first)
        t = torch.from_numpy(x).requires_grad_(True)
        torch.nn.functional.max_pool2d(t[None], 2, 2, ceil_mode=True).backward(torch.from_numpy(g)[None])
        assert _bits(t.grad.numpy(), want)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the gradient: momentum 0, wd 0, lr 1, trunk_layers 5, one step -> w_old - w_new is the gradient plus one rounding of the subtraction
# ---------------------------------------------------------------------------------------------------------------------------------
GRAD_BATCHES = {"B70_two_images": [(33, 9, 0), (37, 11, 1)], "B128_one_image": [(128, 40, 0)], "B1": [(1, 0, 1)]}


@pytest.mark.parametrize("head", HEADS, ids=["fc%d_C%d" % h for h in HEADS])
@pytest.mark.parametrize("case", list(GRAD_BATCHES))
def test_trunk_gradient_against_float64(dev, head, case):
    fc, C = head
    P = _params(fc, C)
    P0 = _np(P)
    net = _net(P)
    _stale(net, dev, C)
    parts = [_batch(1000 + 17 * i + fc, n, C, n_bg, SIZES[sz]) for i, (n, n_bg, sz) in enumerate(GRAD_BATCHES[case])]
    if case == "B1":
        parts = [tuple(a[1:2] if j else a for j, a in enumerate(_batch(1234, 2, C, 0, SIZES[1])))]
    net.train_begin(trunk_layers=5, momentum=0.0, weight_decay=0.0, bbox_weight=1.0)
    for b in parts:
        _add(net, dev, b)
    loss = net.train_step(1.0).cpu().numpy()
    x, images = _device_images(net, dev, parts, 5)
    dx6 = net.debug_tensor("train_dx6", x.shape).cpu().numpy()
    Wd = _weights(net)
    net.train_end()
    rois, gt, labels = _join(parts)
    res = {}
    for dt in (torch.float64, torch.float32):
        tr = TT.Trainer(P0, _trunk_of(P0), POOL, 5, 0.0, 0.0, mean=MEAN, std=STD, dtype=dt)
        l, d = tr.step(x, rois, gt, labels, images, lr=1.0)
        res[dt] = (tr.params(), l, d * (x > 0))
    bad = _judge_all(case, 5, P0, Wd, res[torch.float64][0], res[torch.float32][0], as_difference=True)
    assert (dx6[x <= 0] == 0).all()
    ok, info = _judge("%s dx6" % case, dx6, res[torch.float64][2], res[torch.float32][2])
    if not ok:
        bad.append(info)
    ok, info = _judge("%s loss" % case, loss, np.array(res[torch.float64][1]), np.array(res[torch.float32][1], np.float32), w_new=loss)
    if not ok:
        bad.append(info)
    assert _bits(Wd["conv_w"][0], P0["conv_w"][0]) and _bits(Wd["conv_b"][0], P0["conv_b"][0])   # the first layer: not one bit
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. three steps at lr 1e-3, momentum 0.9, wd 5e-4, a new two-image batch each step, trunk_layers 3, 4, 5
# ---------------------------------------------------------------------------------------------------------------------------------
def _three_steps(net, dev, C, k, lr=1e-3, seed0=2000):
    net.train_begin(trunk_layers=k, momentum=0.9, weight_decay=5e-4, bbox_weight=1.0)
    steps, losses = [], []
    for i in range(3):
        parts = [_batch(seed0 + 2 * i, 40 - 9 * i, C, 8, SIZES[i % 2]), _batch(seed0 + 2 * i + 1, 21 + 4 * i, C, 5, SIZES[(i + 1) % 2])]
        for b in parts:
            _add(net, dev, b)
        losses.append(net.train_step(lr))
        x, images = _device_images(net, dev, parts, k)
        steps.append((x,) + _join(parts) + (images,))
    net.train_end()
    return steps, torch.stack(losses).cpu().numpy()


@pytest.mark.parametrize("k", [3, 4, 5])
def test_three_steps_through_the_pools(dev, k):
    fc, C = HEADS[0]
    P = _params(fc, C)
    P0 = _np(P)
    net = _net(P)
    _stale(net, dev, C)
    steps, losses = _three_steps(net, dev, C, k)
    Wd = _weights(net)
    res = {}
    for dt in (torch.float64, torch.float32):
        tr = TT.Trainer(P0, _trunk_of(P0), POOL, k, 0.9, 5e-4, mean=MEAN, std=STD, dtype=dt)
        ls = [tr.step(*st, lr=1e-3)[0] for st in steps]
        res[dt] = (tr.params(), ls)
    bad = _judge_all("trunk%d" % k, k, P0, Wd, res[torch.float64][0], res[torch.float32][0], as_difference=False)
    ok, info = _judge("trunk%d losses" % k, losses, np.array(res[torch.float64][1]), np.array(res[torch.float32][1], np.float32), w_new=losses)
    if not ok:
        bad.append(info)
    for l in range(NL - k):   # below the trained layers: not one bit
        assert _bits(Wd["conv_w"][l], P0["conv_w"][l]) and _bits(Wd["conv_b"][l], P0["conv_b"][l]), l
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. trunk_layers <= K is depth 2 + trunk_layers: the same bits on a twin handle
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_trunk_layers_up_to_K_are_the_conv_depths(dev, k):
    fc, C = HEADS[1]
    P = _params(fc, C)
    a, b = _net(P), _net(P)
    out = []
    for net, kw in ((a, {"trunk_layers": k}), (b, {"depth": 2 + k})):
        net.train_begin(momentum=0.9, weight_decay=5e-4, **kw)
        ls = []
        for i in range(2):
            _add(net, dev, _batch(5000 + 2 * i, 30, C, 8, SIZES[i % 2]))
            _add(net, dev, _batch(5001 + 2 * i, 17, C, 4, SIZES[(i + 1) % 2]))
            ls.append(net.train_step(1e-2))
        net.train_end()
        out.append((torch.stack(ls).cpu().numpy(), _weights(net)))
    assert _bits(out[0][0], out[1][0]) and _all_bits(out[0][1], out[1][1])
    W0 = _np(P)
    assert not _bits(out[0][1]["conv_w"][NL - k], W0["conv_w"][NL - k]) and _bits(out[0][1]["conv_w"][NL - k - 1], W0["conv_w"][NL - k - 1])


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. lr 0 changes no bit and leaves nothing behind in detect; after a real step every packed form agrees with the exported weights
# ---------------------------------------------------------------------------------------------------------------------------------
def test_lr0_changes_no_bit_and_detect_is_untouched(dev):
    fc, C = HEADS[0]
    net = _net(_params(fc, C))
    im, bx, s0, b0 = _stale(net, dev, C)
    W0 = _weights(net)
    net.train_begin(trunk_layers=5, momentum=0.0, weight_decay=0.0)
    _add(net, dev, _batch(4000, 50, C, 12))
    _add(net, dev, _batch(4001, 30, C, 7, SIZES[1]))
    net.train_step(0.0)
    net.train_end()
    assert _all_bits(_weights(net), W0)
    s1, b1 = net.detect(im, bx)
    assert _bits(s0.cpu().numpy(), s1.cpu().numpy()) and _bits(b0.cpu().numpy(), b1.cpu().numpy())
    fresh = _net(_params(fc, C))   # a handle that never trained (never wrote a pre-pool map) computes the same
    s2, b2 = fresh.detect(im, bx)
    assert _bits(s0.cpu().numpy(), s2.cpu().numpy()) and _bits(b0.cpu().numpy(), b2.cpu().numpy())


def test_packed_forms_agree_with_exported_weights_after_trunk_training(dev):
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
    s1, b1 = [v.clone() for v in net.detect(im, bx)]
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
    W0 = _np(P)
    assert all(not _bits(w, w0) for w, w0 in zip(_weights(net)["conv_w"][1:], W0["conv_w"][1:])) and _bits(_weights(net)["conv_w"][0], W0["conv_w"][0])


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. limits
# ---------------------------------------------------------------------------------------------------------------------------------
def test_trunk_depth_limits(dev):
    from multipathnet_amd import MpnError
    fc, C = HEADS[1]
    net = _net(_params(fc, C))
    W0 = _weights(net)
    for k in (6, 0, 13):   # n_conv: the first layer is never trained; none; beyond MPN_TRAIN_MAX_TRUNK
        with pytest.raises(MpnError) as ei:
            net.train_begin(trunk_layers=k)
        assert "status -1" in str(ei.value) and "MPN_TRAIN_TRUNK(%d)" % k in str(ei.value) and "from 1 to 5" in str(ei.value), str(ei.value)
    with pytest.raises(ValueError):
        net.train_begin(depth=4, trunk_layers=4)
    with pytest.raises(MpnError) as ei:   # MPN_TRAIN_CONV keeps its refusal
        net.train_begin(depth=5)
    assert "K = 2" in str(ei.value) and "pooling layer" in str(ei.value), str(ei.value)
    net.train_begin(trunk_layers=5)
    for i in range(8):
        _add(net, dev, _batch(20 + i, 10, C, 3, SIZES[i % 2]))
    with pytest.raises(MpnError) as ei:
        _add(net, dev, _batch(30, 10, C, 3))
    assert "status -1" in str(ei.value) and "MPN_TRAIN_MAX_IMAGES = 8" in str(ei.value), str(ei.value)
    loss = net.train_step(1e-3).cpu().numpy()   # the eight pending images are still there, and the handle still works
    net.train_end()
    W1 = _weights(net)
    assert np.isfinite(loss).all() and all(np.isfinite(w).all() for w in W1["conv_w"])
    assert _bits(W1["conv_w"][0], W0["conv_w"][0]) and all(not _bits(W1["conv_w"][l], W0["conv_w"][l]) for l in range(1, NL))
    rng = np.random.default_rng(5)
    s, b = net.detect(_t(rng.random((3, H, W), dtype=np.float32), dev), _t(_boxes(rng, 50), dev))
    assert torch.isfinite(s).all() and torch.isfinite(b).all()
