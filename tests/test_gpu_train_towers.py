"""Training MultiPathNet's towers on the device with the trunk frozen (mpn_mpnet_train_*) against float64
(tests/train_towers_np.py).

The float64 side starts from the device's own operands (debug tensors "tower_train_x.<t>"), so the frozen trunk, the ROI pooling and
nn.Normalize are not judged here (test 4 holds the training forward against detect's).  THE YARDSTICK RULE is tests/test_gpu_train.py's: a
device result r is compared with float64 r64 beside the same step(s) done by PyTorch-CPU in fp32 from the same operands, r32:
    e = max(|r - r64| - u |w_new|, 0) elementwise, u = 2^-24,   max(e) <= MARGIN * max|r32 - r64|   and   rms(e) <= MARGIN * rms|r32 - r64|
with MARGIN = 2.0, the value that file chose.  Every comparison prints its two ratios on an `ACC` line.

Two networks, 150 x 250 images, spatial scale 1/16, max_rois 200 (Mp = 256), the five MPN_TOWERS:
  A  cfg [8,16,P,16,24,P,32,32,P,64,P,64]  c3 32, c4 64, c5 64  fc_dim 128  C 5  K 2   detect folds nn.Normalize's scales into the mix GEMM
  B  cfg [8,16,P,16,24,P,24,24,P,40,P,48]  c3 24, c4 40, c5 48  fc_dim 256  C 7  K 1   Kcat 112 pads to 128, c5 to 128; detect normalises in place
K*C is 10 / 7 and 4C 20 / 28: none a multiple of 128, three of them no multiple of 8.  Every handle first runs a 200-ROI detect and (the
gradient test) a 200-row step at lr 0, so rows >= B of every operand hold stale values.

MEASURED on the MI355X (ACC lines of this file; largest max-ratio / rms-ratio over all cases and towers of a test; yardstick = PyTorch-CPU
fp32; DESIGN.md section 13.9 has the same table):
  gradient (6 cases):   mix_w 1.04 / 0.99   mix_b 1.12 / 0.96   fc6_w 1.09 / 0.95   fc6_b 1.01 / 0.93   fc7_w 1.09 / 0.91   fc7_b 1.02 / 0.95
                        cls_w 1.08 / 0.78   cls_b 1.13 / 0.94   bbox_w 1.02 / 1.00  bbox_b 1.03 / 1.00  loss 1.32 / 1.31
  three SGD steps (2):  mix_w 0.63 / 0.28   mix_b 0.56 / 0.37   fc6_w 0.64 / 0.26   fc6_b 0.60 / 0.29   fc7_w 0.63 / 0.26   fc7_b 0.53 / 0.34
                        cls_w 0.92 / 0.53   cls_b 0.79 / 0.78   bbox_w 1.03 / 0.93  bbox_b 0.95 / 0.96  losses 0.90 / 0.93
                        the classifier not selected in steps 0 and 2 (network A): cls_w 0.58 / 0.41, cls_b 0.69 / 0.67
  segmented kernels:    dWmix 0.83 / 0.70   dbmix 1.71 / 1.15   unmasked input gradient 0.87 / 0.74
  forward against detect: network B bit for bit; network A cat 5.6e-7, cls 6.3e-7, bbox 9.7e-7 of max|.| (bound 1e-4)
With ONE chain per bin in the mix weight gradient (B / 2 = 64 dependent MFMA steps) mix_w sat at 2.30 / 1.45 for B = 128; the kernel now
cuts a bin's rows into four quarters added pairwise and is inside 1.04.  The detect side's "bbox_raw" is the regressor's output BEHIND
nn.BBoxNorm (x std + mean), so test 4 puts the training side's raw output through the same two fp32 operations before comparing bits.
Test 3 cannot plant NaN with NaN-free data (and a NaN image would reach the weights even at lr 0): it uses the stale-row set-up."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dropout_np as D  # noqa: E402
import train_kernels_np as R  # noqa: E402
import train_towers_np as TT  # noqa: E402

pytestmark = pytest.mark.gpu

H, W, MAXR, PP = 150, 250, 200, 49
CONFIGS = {
    "A": dict(cfg=[8, 16, "P", 16, 24, "P", 32, 32, "P", 64, "P", 64], c5=64, fc=128, C=5, K=2),
    "B": dict(cfg=[8, 16, "P", 16, 24, "P", 24, 24, "P", 40, "P", 48], c5=48, fc=256, C=7, K=1),
}
NT = 5
STD = [0.1, 0.1, 0.2, 0.2]   # models.synthetic_params' BBoxNorm statistics (mean 0)
MEAN = [0.0, 0.0, 0.0, 0.0]
U = 2.0 ** -24
MARGIN = 2.0   # tests/test_gpu_train.py's


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _params(name, seed=557):
    from multipathnet_amd import models
    c = CONFIGS[name]
    return models.synthetic_mpnet_params(c["cfg"], pooled=7, fc_dim=c["fc"], n_classes=c["C"], n_integral=c["K"], seed=seed)


def _net(P, name, **kw):
    from multipathnet_amd import models
    return models.MultiPathNet(P, cfg=CONFIGS[name]["cfg"], pooled=7, spatial_scale=1.0 / 16, max_h=H, max_w=W, max_rois=MAXR, nms_thresh=0.3, **kw)


def _boxes(rng, n):
    c = rng.uniform([24, 24], [W - 24, H - 24], (n, 2))
    wh = rng.uniform(12, 44, (n, 2))
    return np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)


def _stale(net, dev, seed=99):
    """a detect with max_rois rows: rows >= B of detect's buffers hold values of an earlier, larger call"""
    rng = np.random.default_rng(seed)
    im, bx = _t(rng.random((3, H, W), dtype=np.float32), dev), _t(_boxes(rng, MAXR), dev)
    s, b = net.detect(im, bx)
    torch.cuda.synchronize()
    return im, bx, s, b


def _batch(seed, n, C_, n_bg):
    return TT.make_batch(seed, n, C_, n_bg, H, W)


def _add(net, dev, b):
    net.tower_train_add(_t(b[0], dev), _t(b[1], dev), _t(b[2], dev), _t(b[3], dev))


def _weights(net):
    torch.cuda.synchronize()
    return TT.flat(net.tower_weights())


def _kcat(net):
    return [T["total_feat"] for T in net._towers]


def _operands(net, B):
    return [net.debug_tensor("tower_train_x.%d" % t, (B, kc, PP)).cpu().numpy() for t, kc in enumerate(_kcat(net))]


def _join(parts):
    return np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts])


def _judge(tag, r, r64, r32, w_new=None):
    r, r64, r32 = np.asarray(r, np.float64), np.asarray(r64, np.float64), np.asarray(r32, np.float64)
    assert np.isfinite(r).all(), tag
    e = np.abs(r - r64)
    if w_new is not None:
        e = np.maximum(e - U * np.abs(np.asarray(w_new, np.float64)), 0.0)
    y = np.abs(r32 - r64)
    em, er, ym, yr = float(e.max()), float(np.sqrt((e * e).mean())), float(y.max()), float(np.sqrt((y * y).mean()))
    print("ACC %-28s max e %.3g / torch-fp32 %.3g = %.2f   rms e %.3g / %.3g = %.2f" %
          (tag, em, ym, em / ym if ym else (0.0 if em == 0 else np.inf), er, yr, er / yr if yr else (0.0 if er == 0 else np.inf)))
    return em <= MARGIN * ym and er <= MARGIN * yr, (tag, em, ym, er, yr)


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def _all_bits(Wa, Wb):
    return [n for n in Wa if not _bits(Wa[n], Wb[n])]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the gradient: momentum 0, wd 0, lr 1, one step -> w_old - w_new is the gradient plus one rounding of the subtraction
# ---------------------------------------------------------------------------------------------------------------------------------
GRAD_BATCHES = {"B70_two_images": [(33, 9), (37, 11)], "B128_one_image": [(128, 40)], "B1": [(1, 0)]}


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("case", list(GRAD_BATCHES))
def test_gradient_against_float64(dev, name, case):
    c = CONFIGS[name]
    P = _params(name)
    P0 = TT.flat(P)
    net = _net(P, name)
    _stale(net, dev)
    parts = [_batch(1000 + 17 * i + c["fc"], n, c["C"], n_bg) for i, (n, n_bg) in enumerate(GRAD_BATCHES[case])]
    if case == "B1":
        parts = [tuple(a[1:2] if j else a for j, a in enumerate(_batch(1234, 2, c["C"], 0)))]   # one foreground row with a near GT box
    net.tower_train_begin(momentum=0.0, weight_decay=0.0, bbox_weight=1.0)
    _add(net, dev, _batch(77, MAXR, c["C"], 60))
    net.tower_train_step(0.0)   # max_rois rows at lr 0: the training state's own buffers now hold stale rows too
    assert not _all_bits(_weights(net), P0)
    for b in parts:
        _add(net, dev, b)
    loss = net.tower_train_step(1.0).cpu().numpy()
    rois, gt, labels = _join(parts)
    B = len(labels)
    xs = _operands(net, B)
    Wd = _weights(net)
    net.tower_train_end()
    assert all(np.isfinite(x).all() for x in xs)
    ref = TT.Sgd64(P0, c["K"], momentum=0.0, weight_decay=0.0, mean=MEAN, std=STD)
    l64, d, _ = ref.step(xs, rois, gt, labels, lr=1.0)
    if B > 1:  # both smooth-L1 branches and background rows are really there
        assert (np.abs(d) < 1).any() and (np.abs(d) >= 1).any() and (labels == 0).any() and (labels > 0).any()
    P32, l32 = TT.torch_steps(P0, [(xs, rois, gt, labels, 0, None)], 1.0, c["K"], momentum=0.0, weight_decay=0.0, mean=MEAN, std=STD, dtype=torch.float32)
    bad = []
    for n in TT.names(NT):
        w_old = P0[n].astype(np.float64)
        g64 = w_old - ref.P[n]
        if n == "cls_w" and c["K"] > 1:   # the classifier not selected: an exactly zero gradient; the selected one must not be
            assert (g64[c["C"]:] == 0).all() and _bits(Wd[n][c["C"]:], P0[n][c["C"]:])
            g64_sel = g64[:c["C"]]
        else:
            g64_sel = g64
        assert np.sqrt((g64_sel * g64_sel).mean()) > 0, "%s: the float64 gradient is zero, the case checks nothing" % n
        ok, info = _judge("%s %s %s" % (name, case, n), w_old - Wd[n], g64, w_old - P32[n], w_new=Wd[n])
        if not ok:
            bad.append(info)
    ok, info = _judge("%s %s loss" % (name, case), loss, np.array(l64), np.array(l32[0], np.float32), w_new=loss)
    if not ok:
        bad.append(info)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. three SGD steps at lr 1e-3, momentum 0.9, wd 5e-4, a new batch each step; config A alternates the classifier (0, 1, 0)
# 7. determinism: a second fresh handle, the same steps, every weight bit-identical
# ---------------------------------------------------------------------------------------------------------------------------------
def _three_steps(net, dev, c, lr=1e-3, seed0=2000):
    net.tower_train_begin(momentum=0.9, weight_decay=5e-4, bbox_weight=1.0)
    batches, losses = [], []
    for i in range(3):
        b = _batch(seed0 + i, 66 - 13 * i, c["C"], 12)   # shrinking batches: rows >= B hold the previous step's values
        k = i % c["K"]
        net.tower_train_set_head(k)
        _add(net, dev, b)
        losses.append(net.tower_train_step(lr))
        B = len(b[3])
        g_cls = net.debug_tensor("tower_train_g_cls", (B, c["K"] * c["C"])).cpu().numpy()
        other = np.ones(c["K"] * c["C"], bool)
        other[k * c["C"]:(k + 1) * c["C"]] = False
        assert (g_cls[:, other].view(np.uint32) == 0).all(), "a classifier that was not selected got a gradient (or a -0.0)"
        assert (g_cls[:, ~other] != 0).any()
        batches.append((_operands(net, B), b[1], b[2], b[3], k, None))
    net.tower_train_end()
    return batches, torch.stack(losses).cpu().numpy()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_three_sgd_steps_against_float64(dev, name):
    c = CONFIGS[name]
    P = _params(name)
    P0 = TT.flat(P)
    net = _net(P, name)
    _stale(net, dev)
    batches, losses = _three_steps(net, dev, c)
    Wd = _weights(net)
    ref = TT.Sgd64(P0, c["K"], momentum=0.9, weight_decay=5e-4, mean=MEAN, std=STD)
    l64 = [ref.step(b[0], b[1], b[2], b[3], lr=1e-3, k=b[4])[0] for b in batches]
    P32, l32 = TT.torch_steps(P0, batches, 1e-3, c["K"], momentum=0.9, weight_decay=5e-4, mean=MEAN, std=STD, dtype=torch.float32)
    bad = []
    for n in TT.names(NT):
        assert np.isfinite(Wd[n]).all() and not _bits(Wd[n], P0[n]), n
        ok, info = _judge("%s 3 steps %s" % (name, n), Wd[n], ref.P[n], P32[n], w_new=Wd[n])
        if not ok:
            bad.append(info)
    if c["K"] > 1:   # classifier 1 was selected in the middle step only: decay and momentum alone move it in steps 0 and 2
        rows = slice(c["C"], 2 * c["C"])
        for n in ("cls_w", "cls_b"):
            ok, info = _judge("%s 3 steps %s[k=1]" % (name, n), Wd[n][rows], ref.P[n][rows], P32[n][rows], w_new=Wd[n][rows])
            if not ok:
                bad.append(info)
    ok, info = _judge("%s 3 steps losses" % name, losses, np.array(l64), np.array(l32, np.float32), w_new=losses)
    if not ok:
        bad.append(info)
    assert not bad, bad
    net2 = _net(P, name)
    _stale(net2, dev)
    _, losses2 = _three_steps(net2, dev, c)
    assert _bits(losses, losses2)
    assert not _all_bits(Wd, _weights(net2))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_two_image_step_is_deterministic(dev, name):
    c = CONFIGS[name]
    P = _params(name)
    out = []
    for _ in range(2):
        net = _net(P, name)
        net.tower_train_begin(momentum=0.9, weight_decay=5e-4)
        for i, (n, n_bg) in enumerate(GRAD_BATCHES["B70_two_images"]):
            _add(net, dev, _batch(500 + i, n, c["C"], n_bg))
        loss = net.tower_train_step(0.01).cpu().numpy()
        out.append((loss, _weights(net)))
        net.tower_train_end()
    assert _bits(out[0][0], out[1][0]) and not _all_bits(out[0][1], out[1][1])
    assert all(not _bits(out[0][1][n], TT.flat(P)[n]) for n in TT.names(NT))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. stale rows are never read.  NaN cannot be planted by a step on NaN-free data, and a NaN image would poison the weights even at
#    lr 0 (0 * NaN), so the set-up is the stale-row one: a 200-ROI detect and a 200-row step at lr 0, then B = 3 rows
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_stale_rows_are_never_read(dev, name):
    c = CONFIGS[name]
    P = _params(name)
    b3 = _batch(31, 3, c["C"], 1)
    res = []
    for stale in (True, False):
        net = _net(P, name)
        if stale:
            _stale(net, dev)
        net.tower_train_begin(momentum=0.0, weight_decay=5e-4)
        if stale:
            _add(net, dev, _batch(77, MAXR, c["C"], 60))
            net.tower_train_step(0.0)
            assert not _all_bits(_weights(net), TT.flat(P))
        _add(net, dev, b3)
        loss = net.tower_train_step(0.05).cpu().numpy()
        res.append((loss, _weights(net)))
        net.tower_train_end()
    assert np.isfinite(res[0][0]).all() and all(np.isfinite(v).all() for v in res[0][1].values())
    assert _bits(res[0][0], res[1][0]) and not _all_bits(res[0][1], res[1][1])


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the training forward against detect's, rate 0, the same image and ROIs
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_forward_agrees_with_detect(dev, name):
    c = CONFIGS[name]
    F, KC, C4 = c["fc"], c["K"] * c["C"], 4 * c["C"]
    net = _net(_params(name), name)
    _stale(net, dev)
    b = _batch(41, 70, c["C"], 20)
    net.detect(_t(b[0], dev), _t(b[1], dev))
    det = [net.debug_tensor("cat", (70, NT * F)).cpu().numpy(), net.debug_tensor("cls_k", (70, KC)).cpu().numpy(),
           net.debug_tensor("bbox_raw", (70, C4)).cpu().numpy()]
    net.tower_train_begin(momentum=0.0, weight_decay=0.0)
    _add(net, dev, b)
    net.tower_train_step(0.0)
    trn = [net.debug_tensor("tower_train_cat", (70, NT * F)).cpu().numpy(), net.debug_tensor("tower_train_cls", (70, KC)).cpu().numpy(),
           net.debug_tensor("tower_train_bbox", (70, C4)).cpu().numpy()]
    net.tower_train_end()
    # detect's "bbox_raw" is the regressor's output behind nn.BBoxNorm (d * std + mean, each operation rounded on its own: head_decode_kernel);
    # in training BBoxNorm is the identity, so the training side's raw output goes through the same two fp32 operations first
    std4, mean4 = np.tile(np.array(STD, np.float32), c["C"]), np.tile(np.array(MEAN, np.float32), c["C"])
    trn[2] = (trn[2] * std4[None, :]).astype(np.float32) + mean4[None, :]
    for what, a, d in zip(("cat", "cls", "bbox"), trn, det):
        assert np.isfinite(a).all() and np.abs(d).max() > 0
        err = float(np.abs(a.astype(np.float64) - d).max() / np.abs(d).max())
        print("ACC %s forward %-5s max |train - detect| / max|detect| = %.3g" % (name, what, err))
        if name == "B":   # both sides normalise in place and run the row-invariant GEMMs
            assert _bits(a, d), what
        else:             # detect folds the scales into the mix GEMM: the project's fp32 parity figure
            assert err <= 1e-4, (what, err)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the update is in place, the export is the inverse of creation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_in_place_update_and_export(dev, name):
    c = CONFIGS[name]
    P = _params(name)
    net = _net(P, name)
    assert not _all_bits(_weights(net), TT.flat(P))   # before any step: creation's inputs, bit for bit
    net.set_graphs(True)
    rng = np.random.default_rng(7)
    im, bx = _t(rng.random((3, H, W), dtype=np.float32), dev), _t(_boxes(rng, 90), dev)

    def test_one(n_):
        d, k = n_.test_one_async(im, bx)
        torch.cuda.synchronize()
        return d[: int(k.item())].cpu().numpy().copy()

    for _ in range(4):   # the head and tail chains are captured at the second sighting of the caller's buffers and replayed afterwards
        r0 = test_one(net)
    s0, b0 = net.detect(im, bx)
    replays0 = net.graph_stats()[1]
    assert replays0 > 0
    _three_steps(net, dev, c)
    Wt = net.tower_weights()
    for _ in range(4):
        r1 = test_one(net)
    assert net.graph_stats()[1] > replays0, "no graph was replayed after training"
    s1, b1 = net.detect(im, bx)
    torch.cuda.synchronize()
    assert not _bits(s1.cpu().numpy(), s0.cpu().numpy())
    fresh = _net(Wt, name)
    s2, b2 = fresh.detect(im, bx)
    torch.cuda.synchronize()
    assert _bits(s1.cpu().numpy(), s2.cpu().numpy()) and _bits(b1.cpu().numpy(), b2.cpu().numpy())
    r2 = test_one(fresh)
    assert len(r1) > 0 and _bits(r1, r2), "the replayed graph does not read the trained weights"
    assert not _all_bits(TT.flat(Wt), _weights(fresh))


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. dropout: the masks, their values, reproducibility
# ---------------------------------------------------------------------------------------------------------------------------------
def _dropout_run(dev, name, seed, rate=0.5, lr=1e-3):
    c = CONFIGS[name]
    net = _net(_params(name), name)
    _stale(net, dev)
    net.tower_train_begin(momentum=0.0, weight_decay=0.0, dropout=rate, seed=seed)
    b = _batch(61, 37, c["C"], 9)
    _add(net, dev, b)
    net.tower_train_step(lr)
    B, F = 37, c["fc"]
    y6 = [net.debug_tensor("tower_train_y6.%d" % t, (B, F)).cpu().numpy() for t in range(NT)]
    cat = net.debug_tensor("tower_train_cat", (B, NT * F)).cpu().numpy()
    xs = _operands(net, B)
    Wd = _weights(net)
    return net, b, xs, y6, cat, Wd


def test_dropout_masks_and_values(dev):
    name, seed = "A", 555
    c = CONFIGS[name]
    B, F = 37, c["fc"]
    net, b, xs, y6, cat, Wd = _dropout_run(dev, name, seed)
    net.tower_train_end()
    net0, _, xs0, y60, cat0, _ = _dropout_run(dev, name, seed, rate=0.0)
    net0.tower_train_end()
    assert all(_bits(a, a0) for a, a0 in zip(xs, xs0))
    drop = TT.masks(seed, 0, NT, B, F, 0.5)
    tow, cat64, _, _ = TT.forward({n: v.astype(np.float64) for n, v in TT.flat(_params(name)).items()}, [x.astype(np.float64) for x in xs],
                                  [(a.astype(np.float64), m.astype(np.float64)) for a, m in drop])
    seen = []
    for t in range(NT):
        k6, k7 = drop[t][0] > 0, drop[t][1] > 0
        assert _bits(k6, D.keep_mask(seed, 0, 2 * t, B, F, 0.5)) and _bits(k7, D.keep_mask(seed, 0, 2 * t + 1, B, F, 0.5))
        # behind fc6 the input is the same with and without dropout: kept values are fl(x * 2) exactly, dropped ones +0.0
        assert (y6[t][~k6].view(np.uint32) == 0).all() and _bits(y6[t][k6], y60[t][k6] * np.float32(2.0))
        assert (y6[t][k6] > 0).mean() > 0.2, "too few live elements behind fc6 for the pattern to mean anything"
        y7 = cat[:, t * F:(t + 1) * F]
        assert (y7[~k7].view(np.uint32) == 0).all()
        ref7 = tow[t][4]
        assert ((y7 > 0) == (ref7 > 0))[np.abs(tow[t][3]) > 1e-4].all()   # the kept pattern where fc7's pre-activation is not at the ReLU's edge
        assert np.abs(y7 - ref7).max() <= 1e-4 * np.abs(ref7).max()
        seen += [k6, k7]
    for i in range(len(seen)):
        for j in range(i):
            assert not np.array_equal(seen[i], seen[j]), "two layers share a mask"
    net2, _, _, y6b, catb, Wd2 = _dropout_run(dev, name, seed)      # the same seed: the same bits
    net2.tower_train_end()
    assert _bits(cat, catb) and not _all_bits(Wd, Wd2)
    net3, _, _, _, catc, Wd3 = _dropout_run(dev, name, seed + 1)    # another seed: another run
    net3.tower_train_end()
    assert not _bits(cat, catc) and _all_bits(Wd, Wd3)


def test_rate_zero_after_dropout_reproduces_the_plain_bits(dev):
    name = "B"
    c = CONFIGS[name]
    P = _params(name)
    b = _batch(62, 40, c["C"], 10)
    res = []
    for with_dropout_first in (True, False):
        net = _net(P, name)
        net.tower_train_begin(momentum=0.0, weight_decay=0.0)
        if with_dropout_first:
            net.tower_train_set_dropout(0.5, 9)
            _add(net, dev, b)
            net.tower_train_step(0.0)   # lr 0, momentum 0: the weights keep their bits
            net.tower_train_set_dropout(0.0, 9)
        _add(net, dev, b)
        loss = net.tower_train_step(0.01).cpu().numpy()
        res.append((loss, _weights(net)))
        net.tower_train_end()
    assert _bits(res[0][0], res[1][0]) and not _all_bits(res[0][1], res[1][1])


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. an all-background batch: the box regressor and the het tower see weight decay alone
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_all_background_batch(dev, name):
    c = CONFIGS[name]
    P = _params(name)
    P0 = TT.flat(P)
    net = _net(P, name)
    _stale(net, dev)
    lr, wd = np.float32(0.1), np.float32(5e-4)
    net.tower_train_begin(momentum=0.0, weight_decay=float(wd), bbox_weight=1.0)
    _add(net, dev, _batch(81, 50, c["C"], 50))
    loss = net.tower_train_step(float(lr)).cpu().numpy()
    Wd = _weights(net)
    net.tower_train_end()
    assert loss[1] == 0 and loss[0] > 0
    het = NT - 1
    for n in ["bbox_w", "bbox_b"] + ["t%d.%s" % (het, k) for k in TT.TOWER_TENSORS]:
        w = P0[n].astype(np.float32)
        want = w - lr * (wd * w) if TT.is_weight(n) else w    # each operation rounded on its own; biases never decay
        assert _bits(Wd[n], want), n
    assert all(not _bits(Wd[n], P0[n]) for n in ("cls_w", "cls_b", "t0.mix_w", "t0.mix_b", "t0.fc6_w", "t0.fc7_b"))


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. refusals and state: each names its cause (status -5) and leaves the handle usable
# ---------------------------------------------------------------------------------------------------------------------------------
def _refused(fn, word):
    from multipathnet_amd._lib import MpnError
    with pytest.raises(MpnError) as e:
        fn()
    assert "status -5" in str(e.value) and word in str(e.value), str(e.value)


def test_refusals_and_state(dev):
    from multipathnet_amd import models
    name = "A"
    c = CONFIGS[name]
    P = _params(name)
    rng = np.random.default_rng(3)
    im, bx = _t(rng.random((3, H, W), dtype=np.float32), dev), _t(_boxes(rng, 30), dev)
    b = _batch(91, 20, c["C"], 5)

    def usable(net):
        s, _ = net.detect(im, bx)
        assert torch.isfinite(s).all()
        net.tower_train_begin()
        _add(net, dev, b)
        assert torch.isfinite(net.tower_train_step(1e-3)).all()
        net.tower_train_end()

    # a handle that is not an mpn_mpnet_create handle; a pyramid (only such a handle can hold one)
    plain = models.FastRCNN(models.synthetic_params(c["cfg"], pooled=7, fc_dim=c["fc"], n_classes=c["C"]), cfg=c["cfg"], pooled=7, spatial_scale=1.0 / 16,
                            max_h=H, max_w=W, max_rois=MAXR)
    _refused(lambda: plain.tower_train_begin(), "not an mpn_mpnet_create handle")
    _refused(lambda: plain.tower_weights(), "not an mpn_mpnet_create handle")
    plain.set_scales([120, 150])
    _refused(lambda: plain.tower_train_begin(), "pyramid")
    plain.set_scales([])
    plain.train_begin()
    plain.train_end()
    # MPN_FC_SPLIT3
    s3 = _net(P, name, fc_arith="split3")
    _refused(lambda: s3.tower_train_begin(), "MPN_FC_SPLIT3")
    assert torch.isfinite(s3.detect(im, bx)[0]).all()
    net = _net(P, name)
    # augmentation on
    net.set_augment(True)
    _refused(lambda: net.tower_train_begin(), "augmentation")
    net.set_augment(False)
    usable(net)
    # a pending pipelined tail
    net.test_one_pipelined(im, bx)
    _refused(lambda: net.tower_train_begin(), "pending")
    net.flush()
    usable(net)
    # calls out of order
    _refused(lambda: net.tower_train_end(), "no mpn_mpnet_train_begin")
    _refused(lambda: net.tower_train_step(0.1), "no mpn_mpnet_train_begin")
    _refused(lambda: _add(net, dev, b), "no mpn_mpnet_train_begin")
    _refused(lambda: net.tower_train_set_head(0), "no mpn_mpnet_train_begin")
    _refused(lambda: net.tower_train_set_dropout(0.5), "no mpn_mpnet_train_begin")
    net.tower_train_begin()
    _refused(lambda: net.tower_train_begin(), "already begun")
    _refused(lambda: net.tower_train_step(0.1), "no pending rows")
    net.tower_train_end()
    usable(net)
    # the plain entry points keep refusing a MultiPathNet handle
    _refused(lambda: net.train_begin(), "MultiPathNet")
    usable(net)


# ---------------------------------------------------------------------------------------------------------------------------------
# 10. the segmented kernels and the unmasked input gradient one by one (mpn_debug_* pass-throughs of the debug library)
# ---------------------------------------------------------------------------------------------------------------------------------
F32, F64 = np.float32, np.float64
cf, ci, cs, vp = C.c_float, C.c_int, C.c_size_t, C.c_void_p


@functools.lru_cache(maxsize=None)
def _dbg():
    from multipathnet_amd import _lib
    lib = _lib.load("debug")
    b = [vp, cs]
    lib.mpn_debug_sgd_wgrad_seg_c8.argtypes = b + b + [ci, ci, ci, ci, ci] + b + b + b + [cf, cf, cf]
    lib.mpn_debug_sgd_bias_seg_c8.argtypes = b + [ci, ci, ci, ci] + b + b + [cf, cf]
    lib.mpn_debug_linear_dgrad_c8.argtypes = b + [ci, ci, ci] + b + [ci] + b + b + [ci, cf]
    return lib


class Buf(object):
    """a device buffer; .a = (pointer, element count) as the debug entries take them"""

    def __init__(self, arr):
        arr = np.ascontiguousarray(arr, F32)
        self.shape, self.n = arr.shape, arr.size
        self.t = torch.from_numpy(arr.reshape(-1)).to(torch.device("cuda", 0))
        self.a = (vp(self.t.data_ptr()), self.n)

    def read(self):
        torch.cuda.synchronize()
        return self.t.cpu().numpy().reshape(self.shape).copy()


def _ok(rc):
    assert rc == 0, (rc, _dbg().mpn_last_error().decode())


def _seg_pack(a, Mp, chunks):
    """[nseg, B, N] -> the C8 matrix [chunks][nseg * Mp][8] at row pitch nseg * Mp: NaN in every row outside the segments' first B rows
    and in every lane >= N (read and discarded, or never read)"""
    nseg, B, N = a.shape
    out = np.full((chunks, nseg, Mp, 8), np.nan, F32)
    pad = np.full((nseg, B, chunks * 8), np.nan, F32)
    pad[:, :, :N] = a
    out[:, :, :B, :] = pad.reshape(nseg, B, chunks, 8).transpose(2, 0, 1, 3)
    return out.reshape(chunks, nseg * Mp, 8)


@pytest.mark.parametrize("Mp", [128, 256])
@pytest.mark.parametrize("B", [1, 2, 3, 70])
def test_segmented_mix_gradients(dev, B, Mp):
    lib = _dbg()
    bad = []
    for K in (64, 112, 160):
        for N in (48, 64):
            rng = np.random.default_rng([B, Mp, K, N])
            g, x = R.draw(rng, (PP, B, N)), R.draw(rng, (PP, B, K))
            g_c8, x_c8 = _seg_pack(g, Mp, R.cdiv(N, 8)), _seg_pack(x, Mp, R.k64(K) // 8)
            valid = R.lin_valid(K, N, 1)
            w0 = np.where(valid, R.draw(rng, valid.shape), F32(0)).astype(F32)
            g2, x2 = g.reshape(PP * B, N), x.reshape(PP * B, K)
            dW64, db64 = g2.astype(F64).T @ x2.astype(F64), g2.astype(F64).sum(0)
            dW32 = (torch.from_numpy(g2).t() @ torch.from_numpy(x2)).numpy()    # the yardstick: PyTorch-CPU fp32
            db32 = torch.from_numpy(g2).sum(0).numpy()
            out = []
            for _ in range(2):   # twice: the same bits
                gb, xb = Buf(g_c8), Buf(x_c8)   # (held until the results are read: the launches are asynchronous)
                wb, vb_, pb = Buf(np.zeros_like(w0)), Buf(np.zeros_like(w0)), Buf(np.full(PP * w0.size, np.nan, F32))
                _ok(lib.mpn_debug_sgd_wgrad_seg_c8(*gb.a, *xb.a, Mp, PP, B, N, K, *pb.a, *wb.a, *vb_.a, 1.0, 0.0, 0.0))
                bb, bv = Buf(np.zeros(R.lin_np(N), F32)), Buf(np.zeros(R.lin_np(N), F32))
                _ok(lib.mpn_debug_sgd_bias_seg_c8(*gb.a, Mp, PP, B, N, *bb.a, *bv.a, 1.0, 0.0))
                out.append((wb.read(), vb_.read(), bb.read(), bv.read()))
            assert all(_bits(p, q) for p, q in zip(*out))
            w1, v1, b1, bv1 = out[0]
            assert (v1[~valid].view(np.uint32) == 0).all() and (w1[~valid].view(np.uint32) == 0).all(), "a pad lane of the packing was touched"
            assert (bv1[N:].view(np.uint32) == 0).all() and (b1[N:].view(np.uint32) == 0).all()
            dW = R.lin_unpack(v1, K, N, 1)     # lr 1, momentum 0, wd 0 from zero: v ends as the gradient, w as its negative
            assert _bits(R.lin_unpack(w1, K, N, 1), -dW) and _bits(b1[:N], -bv1[:N])
            for tag, r, r64, r32 in (("dWmix", dW, dW64, dW32), ("dbmix", bv1[:N], db64, db32)):
                ok, info = _judge("seg B%d Mp%d K%d N%d %s" % (B, Mp, K, N, tag), r, r64, r32)
                if not ok:
                    bad.append(info)
            # the step itself on real weights: optim.sgd's chain, each operation rounded on its own
            lr, mom, wd = F32(0.25), F32(0.5), F32(5e-4)
            wb, vb_, pb = Buf(w0), Buf(np.where(valid, F32(0.5) * w0, F32(0))), Buf(np.full(PP * w0.size, np.nan, F32))
            gb, xb = Buf(g_c8), Buf(x_c8)
            _ok(lib.mpn_debug_sgd_wgrad_seg_c8(*gb.a, *xb.a, Mp, PP, B, N, K, *pb.a, *wb.a, *vb_.a, float(lr), float(mom), float(wd)))
            w_ref, v_ref = R.sgd_f32(w0, np.where(valid, F32(0.5) * w0, F32(0)).astype(F32), np.where(valid, v1, F32(0)).astype(F32), lr, mom, wd)
            assert _bits(wb.read()[valid], w_ref[valid]) and _bits(vb_.read()[valid], v_ref[valid])
            assert (wb.read()[~valid].view(np.uint32) == 0).all()
    assert not bad, bad


@pytest.mark.parametrize("B", [1, 33])
def test_unmasked_linear_dgrad(dev, B):
    lib = _dbg()
    K, N, Mp = 48 * 49, 256, 128
    rng = np.random.default_rng([B, 17])
    g, w = R.draw(rng, (B, N)), R.draw(rng, (N, K))
    g_c8 = R.c8_pack(g, Mp, lane_fill=np.nan, row_fill=np.nan)
    wpk = R.lin_pack(w, 49)
    act = R.draw(rng, (B, K))      # positive, negative and exact zeros
    chunks = R.cdiv(K, 8)

    def run(act_c8, scale=1.0):
        dx, gb, wb = Buf(np.full((chunks, Mp, 8), np.nan, F32)), Buf(g_c8), Buf(wpk)
        ab = Buf(act_c8) if act_c8 is not None else None
        _ok(lib.mpn_debug_linear_dgrad_c8(*gb.a, Mp, B, N, *wb.a, K, *(ab.a if ab else (None, 0)), *dx.a, Mp, scale))
        return dx.read()

    plain = run(None)
    assert _bits(plain, run(None)) and np.isfinite(plain[:, :B]).all() and np.isnan(plain[:, B:]).all()   # rows >= B: not written
    # against float64 in fc6's chunk order, beside PyTorch-CPU fp32
    kidx = R.lin_k_index(K, 49)[:chunks]
    dx64, dx32 = g.astype(F64) @ w.astype(F64), (torch.from_numpy(g) @ torch.from_numpy(w)).numpy()
    got = np.empty((B, K), F32)
    got[:, kidx.reshape(-1)] = plain[:, :B, :].transpose(1, 0, 2).reshape(B, -1)
    ok, info = _judge("dgrad unmasked B%d" % B, got, dx64, dx32)
    assert ok, info
    # the masked form: the unmasked result where act > 0, +0.0 elsewhere — the mask only selects
    act_c8 = R.x_pack(act, 49, Mp)[:chunks]
    masked = run(act_c8)
    want = np.where(act_c8[:, :B] > 0, plain[:, :B], F32(0))
    assert _bits(masked[:, :B], want) and (act > 0).any() and (act <= 0).any()
    assert _bits(run(act_c8, 2.0)[:, :B], want * F32(2.0))


def test_masked_dgrad_is_the_unmasked_one_selected(dev):
    """one shape of tests/test_gpu_train_kernels_numerics.py's (its inputs, its pitches; that file pins the masked form's bits): the masked
    result equals the unmasked one where act > 0 and is +0.0 elsewhere (-0.0, NaN and negative activations included) — exact, the mask selects"""
    lib = _dbg()
    N, K, B, g_mp, x_mp = 35, 96, 70, 136, 104
    assert (N, K, B) in R.dgrad_cases()
    g, w, act = R.dgrad_inputs(N, K, B)
    g_c8, wpk, act_c8 = R.c8_pack(g, g_mp, lane_fill=np.nan, row_fill=np.nan), R.lin_pack(w, 1, fill=np.nan), R.c8_pack(act, x_mp, row_fill=np.nan)
    res = []
    gb, wb, ab = Buf(g_c8), Buf(wpk), Buf(act_c8)
    for a in (ab.a, (None, 0)):
        dx = Buf(np.full((K // 8, x_mp, 8), np.nan, F32))
        _ok(lib.mpn_debug_linear_dgrad_c8(*gb.a, g_mp, B, N, *wb.a, K, *a, *dx.a, x_mp, 1.0))
        res.append(R.c8_unpack(dx.read(), B, K))
    masked, plain = res
    assert np.isfinite(plain).all() and (plain != 0).any()
    assert _bits(masked, np.where(act > 0, plain, F32(0)))
