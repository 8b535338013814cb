"""Training the Fast R-CNN head on the device (mpn_frcnn_train_*) against float64 (tests/train_np.py).

The float64 side starts from the device's own pooled operand (debug tensor "train_pooled"), so the frozen trunk is not judged here.
THE YARDSTICK RULE: a device result r (a weight tensor, a weight difference, a loss curve) is compared with float64 r64 beside the
same step(s) done by PyTorch-CPU in fp32 (autograd + torch.optim.SGD from the same pooled operand), r32:
    e = max(|r - r64| - u |w_new|, 0) elementwise, u = 2^-24 (the derivable cost of the final fp32 subtraction w - lr v),
    max(e) <= MARGIN * max|r32 - r64|   and   rms(e) <= MARGIN * rms|r32 - r64|.
Every comparison prints its two ratios on an `ACC` line.  MARGIN started from the 1.5 x that tests/test_gpu_gemm_numerics.py grants over
the oracle's chain; the ratios measured on the MI355X and the margin chosen over them are recorded at MARGIN below and in DESIGN.md
section 13.

Network: cfg [8, 16, P, 16, P, 32], 7 x 7 pooling (K6 = 1568), spatial scale 1/4, 96 x 160 images, max_rois 200; heads (fc_dim 96, C 7) —
NP pads 96 -> 128, 5C = 35 is neither a multiple of 8 nor of 128 — and (fc_dim 128, C 4).  Every handle first runs a detect with 200
ROIs, and the gradient test a 200-row training step at lr 0 (the minibatch has activation buffers of its own), so rows >= B of every
operand buffer hold stale values."""
import numpy as np
import pytest
import torch

import train_np as T

pytestmark = pytest.mark.gpu

CFG = [8, 16, "P", 16, "P", 32]
H, W, MAXR, K6 = 96, 160, 200, 32 * 49
HEADS = [(96, 7), (128, 4)]
STD = [0.1, 0.1, 0.2, 0.2]   # models.synthetic_params' BBoxNorm statistics (mean 0)
MEAN = [0.0, 0.0, 0.0, 0.0]
U = 2.0 ** -24
# MEASURED on MI355X (ACC lines of this file; largest max-ratio / rms-ratio over all cases of a test; yardstick = PyTorch-CPU fp32):
#   gradient (6 cases):  fc6_w 0.64 / 0.64   fc6_b 0.88 / 0.66   fc7_w 1.10 / 0.67   fc7_b 0.66 / 0.59   cls_w 1.32 / 0.81   cls_b 0.25 / 0.24
#                        bbox_w 1.20 / 1.32   bbox_b 1.17 / 1.33   loss 1.25 / 1.25
#   three SGD steps (6): fc6_w 0.62 / 0.26   fc6_b 0.53 / 0.34   fc7_w 0.54 / 0.25   fc7_b 0.58 / 0.35   cls_w 0.53 / 0.28   cls_b 0.41 / 0.40
#                        bbox_w 1.10 / 0.73   bbox_b 0.50 / 0.40   losses 0.63 / 0.49
#   saturated L_cls 0.00 (exact)        30-step loss curve (lr 0.01) 0.48 / 0.35
# The largest is 1.33 (the B = 1 cases, where one fp32 product's rounding is all there is on either side).  MARGIN = 2.0 leaves 1.5 x
# head-room over it: the yardstick itself moves with the CPU whose BLAS blocks the fp32 sums (it is a sample of fp32's error, not a
# bound), while the device's orders are fixed — 64 sequential row pairs in the MFMA chain where a blocked CPU sum has shorter chains.
# (With a row-ascending bias sum the bias gradients sat at 1.9 - 3.3; the kernel sums pairwise now and is inside 1.0.)
MARGIN = 2.0


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _params(fc, C, seed=557, head_scale="trained"):
    from multipathnet_amd import models
    return models.synthetic_params(CFG, pooled=7, fc_dim=fc, n_classes=C, seed=seed, head_scale=head_scale)


def _np(P):
    return {k: np.asarray(P[k].detach().cpu().numpy() if hasattr(P[k], "detach") else P[k]) for k in T.TENSORS}


def _net(P, **kw):
    from multipathnet_amd import models
    return models.FastRCNN(P, cfg=CFG, pooled=7, spatial_scale=0.25, max_h=H, max_w=W, max_rois=MAXR, nms_thresh=0.3, **kw)


def _boxes(rng, n):
    c = rng.uniform([24, 24], [W - 24, H - 24], (n, 2))
    wh = rng.uniform(12, 44, (n, 2))
    return np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)


def _stale(net, dev, seed=99):
    """a detect with max_rois rows: rows >= B of x6 / y6 / y7 / head hold values of an earlier, larger call"""
    rng = np.random.default_rng(seed)
    im, bx = _t(rng.random((3, H, W), dtype=np.float32), dev), _t(_boxes(rng, MAXR), dev)
    s, b = net.detect(im, bx)
    torch.cuda.synchronize()
    return im, bx, s, b


def _batch(seed, n, C, n_bg):
    """one image's rows: the first n_bg background; of the foreground rows every third regresses to a GT box half a box width away
    (normalised |d| >= 1, the linear branch), the others to a GT box within a pixel (|d| < 1, the quadratic branch)"""
    rng = np.random.default_rng(seed)
    im = rng.random((3, H, W), dtype=np.float32)
    rois = _boxes(rng, n)
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
    return {k: v.cpu().numpy() for k, v in net.head_weights().items()}


def _pooled(net, B):
    return net.debug_tensor("train_pooled", (B, K6)).cpu().numpy()


def _join(parts):
    return np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts])


def _judge(tag, r, r64, r32, w_new=None, margin=None):
    margin = MARGIN if margin is None else margin
    r, r64, r32 = np.asarray(r, np.float64), np.asarray(r64, np.float64), np.asarray(r32, np.float64)
    e = np.abs(r - r64)
    if w_new is not None:
        e = np.maximum(e - U * np.abs(np.asarray(w_new, np.float64)), 0.0)
    y = np.abs(r32 - r64)
    em, er, ym, yr = float(e.max()), float(np.sqrt((e * e).mean())), float(y.max()), float(np.sqrt((y * y).mean()))
    print("ACC %-28s max e %.3g / torch-fp32 %.3g = %.2f   rms e %.3g / %.3g = %.2f" %
          (tag, em, ym, em / ym if ym else (0.0 if em == 0 else np.inf), er, yr, er / yr if yr else (0.0 if er == 0 else np.inf)))
    return em <= margin * ym and er <= margin * yr, (tag, em, ym, er, yr)


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the gradient: momentum 0, wd 0, lr 1, depth 2, one step -> w_old - w_new is the gradient plus one rounding of the subtraction
# ---------------------------------------------------------------------------------------------------------------------------------
GRAD_BATCHES = {"B70_two_images": [(33, 9), (37, 11)], "B128_one_image": [(128, 40)], "B1": [(1, 0)]}


@pytest.mark.parametrize("head", HEADS, ids=["fc%d_C%d" % h for h in HEADS])
@pytest.mark.parametrize("case", list(GRAD_BATCHES))
def test_gradient_against_float64(dev, head, case):
    fc, C = head
    P = _params(fc, C)
    P0 = _np(P)
    net = _net(P)
    _stale(net, dev)
    parts = [_batch(1000 + 17 * i + fc, n, C, n_bg) for i, (n, n_bg) in enumerate(GRAD_BATCHES[case])]
    if case == "B1":
        parts = [tuple(a[1:2] if j else a for j, a in enumerate(_batch(1234, 2, C, 0)))]   # one foreground row with a near GT box
    net.train_begin(depth=2, momentum=0.0, weight_decay=0.0, bbox_weight=1.0)
    _add(net, dev, _batch(77, MAXR, C, 60))
    net.train_step(0.0)   # max_rois rows at lr 0 (no momentum: nothing is carried over): the minibatch's own buffers now hold stale rows too
    assert all(_bits(v, P0[k]) for k, v in _weights(net).items())
    for b in parts:
        _add(net, dev, b)
    loss = net.train_step(1.0).cpu().numpy()
    rois, gt, labels = _join(parts)
    B = len(labels)
    x = _pooled(net, B)
    Wd = _weights(net)
    net.train_end()
    ref = T.Sgd64(P0, depth=2, momentum=0.0, weight_decay=0.0, mean=MEAN, std=STD)
    l64, d = ref.step(x, rois, gt, labels, lr=1.0)
    if B > 1:  # both smooth-L1 branches and background rows are really there
        assert (np.abs(d) < 1).any() and (np.abs(d) >= 1).any() and (labels == 0).any() and (labels > 0).any()
    P32, l32 = T.torch_steps(P0, [(x, rois, gt, labels)], 1.0, depth=2, momentum=0.0, weight_decay=0.0, mean=MEAN, std=STD, dtype=torch.float32)
    bad = []
    for k in T.TENSORS:
        w_old = P0[k].astype(np.float64)
        ok, info = _judge("%s %s" % (case, k), w_old - Wd[k], w_old - ref.P[k], w_old - P32[k], w_new=Wd[k])
        if not ok:
            bad.append(info)
    ok, info = _judge("%s loss" % case, loss, np.array(l64), np.array(l32[0], np.float32), w_new=loss)
    if not ok:
        bad.append(info)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. optimiser semantics + 5. reproducibility: three steps at lr 1e-3, momentum 0.9, wd 5e-4, a new batch each step, every depth
# ---------------------------------------------------------------------------------------------------------------------------------
def _three_steps(net, dev, C, depth, lr=1e-3, seed0=2000):
    net.train_begin(depth=depth, momentum=0.9, weight_decay=5e-4, bbox_weight=1.0)
    batches, losses = [], []
    for i in range(3):
        b = _batch(seed0 + i, 66 - 13 * i, C, 12)   # shrinking batches: rows >= B hold the previous step's values
        _add(net, dev, b)
        losses.append(net.train_step(lr))
        batches.append((_pooled(net, len(b[3])), b[1], b[2], b[3]))
    net.train_end()
    return batches, torch.stack(losses).cpu().numpy()


@pytest.mark.parametrize("head", HEADS, ids=["fc%d_C%d" % h for h in HEADS])
@pytest.mark.parametrize("depth", [0, 1, 2])
def test_three_sgd_steps_against_float64(dev, head, depth):
    fc, C = head
    P = _params(fc, C)
    P0 = _np(P)
    net = _net(P)
    _stale(net, dev)
    batches, losses = _three_steps(net, dev, C, depth)
    Wd = _weights(net)
    ref = T.Sgd64(P0, depth=depth, momentum=0.9, weight_decay=5e-4, mean=MEAN, std=STD)
    l64 = [ref.step(*b, lr=1e-3)[0] for b in batches]
    P32, l32 = T.torch_steps(P0, batches, 1e-3, depth=depth, momentum=0.9, weight_decay=5e-4, mean=MEAN, std=STD, dtype=torch.float32)
    bad = []
    for k in T.TENSORS:
        if k not in T.TRAINED[depth]:
            assert _bits(Wd[k], P0[k]), "%s is outside depth %d and changed" % (k, depth)
            continue
        assert np.isfinite(Wd[k]).all() and not _bits(Wd[k], P0[k]), k
        ok, info = _judge("depth%d %s" % (depth, k), Wd[k], ref.P[k], P32[k], w_new=Wd[k])
        if not ok:
            bad.append(info)
    ok, info = _judge("depth%d losses" % depth, losses, np.array(l64), np.array(l32, np.float32), w_new=losses)
    if not ok:
        bad.append(info)
    assert not bad, bad
    # 5. a second fresh handle, the same three steps: every weight bit-identical
    net2 = _net(P)
    _stale(net2, dev)
    _, losses2 = _three_steps(net2, dev, C, depth)
    W2 = _weights(net2)
    assert _bits(losses, losses2)
    for k in T.TENSORS:
        assert _bits(Wd[k], W2[k]), k


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. an all-background batch: no box loss, no box gradient, biases do not decay
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", HEADS, ids=["fc%d_C%d" % h for h in HEADS])
def test_all_background_batch(dev, head):
    fc, C = head
    P = _params(fc, C)
    P0 = _np(P)
    net = _net(P)
    _stale(net, dev)
    lr, wd = 1e-3, 5e-4
    net.train_begin(depth=2, momentum=0.9, weight_decay=wd, bbox_weight=1.0)
    b = _batch(3000, 50, C, 50)
    assert (b[3] == 0).all()
    _add(net, dev, b)
    loss = net.train_step(lr).cpu().numpy()
    Wd = _weights(net)
    net.train_end()
    assert loss[1] == 0.0 and np.isfinite(loss[0]) and loss[0] > 0
    # the box rows of the gradient are exactly zero: the weights see the decay alone (each operation rounded on its own), the bias nothing
    want = P0["bbox_w"] - np.float32(lr) * (np.float32(wd) * P0["bbox_w"])
    assert _bits(Wd["bbox_w"], want.astype(np.float32))
    assert _bits(Wd["bbox_b"], P0["bbox_b"])
    assert not _bits(Wd["cls_b"], P0["cls_b"]) and not _bits(Wd["fc6_w"], P0["fc6_w"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. saturated logits (|z| ~ 40): log-sum-exp keeps the loss finite and accurate
# ---------------------------------------------------------------------------------------------------------------------------------
def test_saturated_logits(dev):
    fc, C = HEADS[0]
    P = _params(fc, C)
    b = _batch(4000, 64, C, 20)
    probe = _net(P)
    _stale(probe, dev)
    probe.train_begin(depth=0, momentum=0.0, weight_decay=0.0)
    _add(probe, dev, b)
    probe.train_step(0.0)
    x = _pooled(probe, 64)
    probe.train_end()
    z = T.forward({k: v.astype(np.float64) for k, v in _np(P).items()}, x.astype(np.float64))[2]
    s = 40.0 / np.abs(z).max()
    Q = dict(P)
    Q["cls_w"], Q["cls_b"] = P["cls_w"] * float(s), P["cls_b"] * float(s)
    Q0 = _np(Q)
    net = _net(Q)
    _stale(net, dev)
    net.train_begin(depth=2, momentum=0.9, weight_decay=5e-4)
    _add(net, dev, b)
    loss = net.train_step(1e-3).cpu().numpy()
    x = _pooled(net, 64)
    Wd = _weights(net)
    net.train_end()
    ref = T.Sgd64(Q0, depth=2, momentum=0.9, weight_decay=5e-4, mean=MEAN, std=STD)
    l64, _ = ref.step(x, b[1], b[2], b[3], lr=1e-3)
    z64 = T.forward({k: v.astype(np.float64) for k, v in Q0.items()}, x.astype(np.float64))[2]
    assert 39.0 <= np.abs(z64).max() <= 41.0
    P32, l32 = T.torch_steps(Q0, [(x, b[1], b[2], b[3])], 1e-3, depth=2, momentum=0.9, weight_decay=5e-4, mean=MEAN, std=STD, dtype=torch.float32)
    assert np.isfinite(loss).all() and loss[0] > 1.0
    for k in T.TENSORS:
        assert np.isfinite(Wd[k]).all(), k
    ok, info = _judge("saturated L_cls", loss[:1], np.array(l64[:1]), np.array(l32[0][:1], np.float32), w_new=loss[:1])
    assert ok, info


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the weights are updated in place: detect, a graph captured BEFORE training, and a new handle made from head_weights() agree
# ---------------------------------------------------------------------------------------------------------------------------------
def test_in_place_update_is_what_detect_and_captured_graphs_read(dev):
    fc, C = HEADS[0]
    P = _params(fc, C)
    net = _net(P)
    net.set_graphs(True)
    im, bx, s0, b0 = _stale(net, dev)
    for _ in range(3):   # the head and tail graphs are captured at the second sighting of these buffers and replayed at the third
        net.test_one_async(im, bx)
    torch.cuda.synchronize()
    cap0, rep0 = net.graph_stats()
    assert cap0 >= 1 and rep0 >= 1
    _three_steps(net, dev, C, 2, lr=1e-2)
    s1, b1 = net.detect(im, bx)
    runs = []
    for _ in range(3):   # the first runs for real (training rewrote the head's buffers), the later ones replay the graphs captured before training
        d, n = net.test_one_async(im, bx)
        torch.cuda.synchronize()
        runs.append((d.cpu().numpy().copy(), int(n.item())))
    cap1, rep1 = net.graph_stats()
    assert cap1 == cap0 and rep1 > rep0, "the graphs captured before training were not replayed"
    W1 = net.head_weights()
    Pn = dict(P)
    Pn.update({k: v.cpu() for k, v in W1.items()})
    fresh = _net(Pn)
    s2, b2 = fresh.detect(im, bx)
    d2, n2 = fresh.test_one_async(im, bx)
    torch.cuda.synchronize()
    assert _bits(s1.cpu().numpy(), s2.cpu().numpy()) and _bits(b1.cpu().numpy(), b2.cpu().numpy())
    n2 = int(n2.item())
    assert n2 > 0
    for d, n in runs:
        assert n == n2 and _bits(d[:min(n, d.shape[0])], d2.cpu().numpy()[:min(n2, d.shape[0])])
    W2 = _weights(fresh)   # unpack -> create -> unpack
    for k in T.TENSORS:
        assert _bits(W1[k].cpu().numpy(), W2[k]), k
    assert not _bits(s0.cpu().numpy(), s1.cpu().numpy()), "training did not change what detect computes"


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. convergence: depth 0, 30 steps on one fixed batch; the device's loss curve follows float64's
# ---------------------------------------------------------------------------------------------------------------------------------
def test_loss_curve_follows_float64(dev):
    fc, C = HEADS[0]
    P = _params(fc, C, head_scale="init")
    P0 = _np(P)
    net = _net(P)
    _stale(net, dev)
    b = _batch(7000, 64, C, 24)
    net.train_begin(depth=0, momentum=0.0, weight_decay=0.0)
    _add(net, dev, b)
    net.train_step(0.0)   # lr 0 without momentum changes nothing: it only leaves the pooled operand to read
    x = _pooled(net, 64)
    assert all((v == P0[k]).all() for k, v in _weights(net).items())   # (by value: the initialisation's zero biases carry both signs of zero)
    lr = None
    for cand in (1.0, 0.3, 0.1, 0.03, 0.01, 0.003):   # the largest of these at which float64's total loss falls at every step
        ref = T.Sgd64(P0, depth=0, momentum=0.0, weight_decay=0.0, mean=MEAN, std=STD)
        curve = np.array([ref.step(x, b[1], b[2], b[3], lr=cand)[0] for _ in range(30)])
        if (np.diff(curve.sum(1)) < 0).all():
            lr = cand
            break
    assert lr is not None
    dev_curve = []
    for _ in range(30):
        _add(net, dev, b)
        dev_curve.append(net.train_step(lr))
    dev_curve = torch.stack(dev_curve).cpu().numpy()
    net.train_end()
    _, l32 = T.torch_steps(P0, [(x, b[1], b[2], b[3])] * 30, lr, depth=0, momentum=0.0, weight_decay=0.0, mean=MEAN, std=STD, dtype=torch.float32)
    assert dev_curve.sum(1)[-1] < dev_curve.sum(1)[0] and np.isfinite(dev_curve).all()
    ok, info = _judge("30-step loss curve lr %g" % lr, dev_curve, curve, np.array(l32, np.float32), w_new=dev_curve)
    assert ok, info


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. refusals and state
# ---------------------------------------------------------------------------------------------------------------------------------
def test_handles_that_cannot_train_refuse_with_a_message(dev):
    from multipathnet_amd import MpnError, models
    big = [8, 16, "P", 16, 24, "P", 32, 32, "P", 64, "P", 64]
    mp = models.synthetic_mpnet_params(big, pooled=7, fc_dim=128, n_classes=5, n_integral=2, seed=11)
    R = models.synthetic_resnet_params(depth=0, n_classes=5, base_width=8, blocks=[1, 1, 1, 1], block_type="bottleneck", seed=3)
    G = models.synthetic_alexnet_params(n_classes=6, seed=5, width=0.25, fc_dim=256)
    kinds = [("MultiPathNet", lambda: models.MultiPathNet(mp, cfg=big, pooled=7, spatial_scale=1 / 16, max_h=150, max_w=250, max_rois=32)),
             ("ResNet", lambda: models.ResNetFRCNN(R, max_h=150, max_w=250, max_rois=32, top_k=10)),
             ("op-list", lambda: models.AlexNetFRCNN(G, max_h=160, max_w=209, max_rois=32, top_k=10)),
             ("SPLIT3", lambda: _net(_params(*HEADS[1]), fc_arith="split3"))]
    for word, mk in kinds:
        h = mk()
        for call in (lambda: h.train_begin(), lambda: h.train_step(0.1), lambda: h.train_end() if word == "SPLIT3" else h.train_begin(depth=0)):
            with pytest.raises(MpnError) as ei:
                call()
            assert "status -5" in str(ei.value) and (word in str(ei.value) or "no mpn_frcnn_train_begin" in str(ei.value)), str(ei.value)
        h.close()
    net = _net(_params(*HEADS[1]))
    net.set_scales([80, 96])
    with pytest.raises(MpnError) as ei:
        net.train_begin()
    assert "status -5" in str(ei.value) and "pyramid" in str(ei.value)
    net.set_scales([])
    net.set_augment(True)
    with pytest.raises(MpnError) as ei:
        net.train_begin()
    assert "status -5" in str(ei.value) and "augmentation" in str(ei.value)
    net.set_augment(False)
    im, bx, _, _ = _stale(net, dev)
    net.test_one_pipelined(im, bx)
    with pytest.raises(MpnError) as ei:
        net.train_begin()
    assert "status -5" in str(ei.value) and "mpn_frcnn_flush" in str(ei.value)
    net.flush()
    net.train_begin()
    net.train_end()


def test_state_errors_leave_the_handle_usable(dev):
    from multipathnet_amd import MpnError
    fc, C = HEADS[1]
    net = _net(_params(fc, C))
    im, bx, s0, b0 = _stale(net, dev)
    with pytest.raises(MpnError) as ei:   # no begin yet
        net.train_step(0.1)
    assert "status -5" in str(ei.value)
    net.train_begin(depth=2)
    with pytest.raises(MpnError) as ei:
        net.train_begin(depth=2)
    assert "status -5" in str(ei.value) and "already" in str(ei.value)
    with pytest.raises(MpnError) as ei:
        net.train_step(0.1)
    assert "status -5" in str(ei.value) and "pending" in str(ei.value)
    _add(net, dev, _batch(8000, 150, C, 50))
    with pytest.raises(MpnError) as ei:
        _add(net, dev, _batch(8001, 51, C, 10))
    assert "status -1" in str(ei.value) and "max_rois" in str(ei.value)
    # the trunk's cached map now belongs to the training image: a detect on cached features must not pool from it
    with pytest.raises(MpnError) as ei:
        net.detect(im, bx, recompute_features=False)
    assert "no cached" in str(ei.value)
    s1, b1 = net.detect(im, bx)   # no step was taken: the weights are what they were
    assert _bits(s0.cpu().numpy(), s1.cpu().numpy()) and _bits(b0.cpu().numpy(), b1.cpu().numpy())
    s1c, _ = net.detect(im, bx, recompute_features=False)   # and the handle caches features again
    assert _bits(s1.cpu().numpy(), s1c.cpu().numpy())
    net.train_step(1e-2)          # the 150 pending rows are still there
    s2, b2 = net.detect(im, bx)
    net.train_end()
    with pytest.raises(MpnError):
        net.train_end()
    s3, b3 = net.detect(im, bx)   # after train_end: still runs, on the trained weights
    assert _bits(s2.cpu().numpy(), s3.cpu().numpy()) and _bits(b2.cpu().numpy(), b3.cpu().numpy())
    assert not _bits(s0.cpu().numpy(), s3.cpu().numpy())
