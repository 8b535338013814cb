"""MultiPathNet's conv5 block trained through the skip pooling on the device (mpn_mpnet_train_begin_conv)
against float64 (tests/train_phase2_np.py).

The float64 side starts from what the device saved for its own backward pass — the block's input map, the ReLU masks of the trained
layers' outputs, the argmax of every Foveal region, the conv4 / conv3 slabs of the operands — so the frozen part of the trunk and the
choice of a maximum are not judged here (the argmax is held against tests/train_conv_np.py own_argmax on the device's map, bit for
bit).  THE YARDSTICK RULE is tests/test_gpu_train.py's, with its MARGIN = 2.0: a device result r beside float64 r64 and the same step(s)
by PyTorch-CPU in fp32 from the same saved maps, argmax and masks, r32:
    e = max(|r - r64| - u |w_new|, 0),   max(e) <= MARGIN * max|r32 - r64|   and   rms(e) <= MARGIN * rms|r32 - r64|.
150 x 250 images, max_rois 200, the five MPN_TOWERS (regions 0, 1, 2, 3, 1: towers 1 and 4 share an argmax), pooled 7 x 7:
  B  tests/test_gpu_train_towers.py's network B, K = 1: conv 40 -> 48 trained
  C  cfg [8,16,P,16,24,P,24,24,P,40,P,48,12,48], K = 3: conv 40 -> 48 -> 12 -> 48 trained; the 12-channel layer has no Winograd form in
     the forward, and 12 is no multiple of 8; fc_dim 128, C 5, K 2 classifiers
Every handle first runs a 200-ROI detect; the gradient tests (momentum 0, wd 0: it leaves no trace in the optimiser) also a 200-row step
at lr 0, so rows >= B of every buffer, the training state's included, hold stale values.

The tests that fail on the parent commit: all of them (tower_train_begin has no conv_layers there), test_conv_layers_0_* included.

MEASURED on the MI355X (ACC lines of this file; largest max-ratio / rms-ratio over the cases of a test; yardstick = PyTorch-CPU fp32;
DESIGN.md section 13.15 has the same table):
  gradient (5 cases):  mix_w 1.25 / 0.98  mix_b 1.17 / 0.94  fc6_w 1.44 / 0.95  fc6_b 1.06 / 0.91  fc7_w 1.05 / 0.91  fc7_b 0.97 / 0.92
                       cls_w 1.25 / 0.88  cls_b 1.40 / 1.15  bbox_w 1.00 / 1.01  bbox_b 1.01 / 0.99  loss 1.00 / 0.86
                       conv_w.7 1.14 / 1.07  conv_w.8 1.71 / 1.02  conv_w.9 0.77 / 0.82  conv_b.7 1.19 / 1.13  conv_b.8 1.53 / 1.17  conv_b.9 0.81 / 0.85
  three SGD steps (2): tower and head tensors <= 1.14 / 1.01 (bbox_w), conv_w <= 0.53 / 0.26, conv_b <= 0.42 / 0.29, losses 0.57 / 0.44
  dx5 against float64: largest err / bound 0.27
With the block's input gradients on the forward's Winograd kernel, as the plain handle runs them, conv_w.8 (network C's 48 -> 12 layer,
whose output gradient is layer 9's input gradient) measured 2.52 / 1.10 at B = 70 over two images: over the margin.  The tower handle's
block therefore runs its input gradients on the direct kernels (1.71 / 1.02 above); the margin is what it was."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_conv_np as TC  # noqa: E402
import train_phase2_np as P2  # noqa: E402
import train_towers_np as TT  # noqa: E402
from train_phase2_np import H, W, MAXR, PP, NETS, NT, REGIONS, GRAD_BATCHES, STD, MEAN, SCALE  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
MARGIN = 2.0   # tests/test_gpu_train.py's


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _net(P, name, **kw):
    from multipathnet_amd import models
    return models.MultiPathNet(P, cfg=NETS[name]["cfg"], pooled=7, spatial_scale=SCALE, max_h=H, max_w=W, max_rois=MAXR, nms_thresh=0.3, **kw)


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def _weights(net):
    """the flat dict of every tower / head tensor and every conv tensor of the trunk"""
    torch.cuda.synchronize()
    Wt = TT.flat(net.tower_weights())
    tw = net.trunk_weights()
    for l in range(len(tw["conv_w"])):
        Wt["conv_w.%d" % l], Wt["conv_b.%d" % l] = tw["conv_w"][l].cpu().numpy(), tw["conv_b"][l].cpu().numpy()
    return Wt


def _diff(Wa, Wb):
    return [n for n in Wa if not _bits(Wa[n], Wb[n])]


def _stale(net, dev, c, conv_layers, lr0_step=True, **kw):
    """a 200-ROI detect, train_begin and (lr0_step: at momentum 0 and wd 0 it leaves no trace in the optimiser) a 200-row step at lr 0:
    rows >= B of every buffer, the training state's included, hold stale values"""
    rng = np.random.default_rng(99)
    c_ = rng.uniform([24, 24], [W - 24, H - 24], (MAXR, 2))
    wh = rng.uniform(12, 44, (MAXR, 2))
    net.detect(_t(rng.random((3, H, W), dtype=np.float32), dev), _t(np.concatenate([c_ - wh / 2, c_ + wh / 2], 1).astype(np.float32), dev))
    W0 = _weights(net)
    net.tower_train_begin(conv_layers=conv_layers, **kw)
    if lr0_step:
        _add(net, dev, P2.batch(77, MAXR, c["C"], 60))
        net.tower_train_step(0.0)
        assert not _diff(_weights(net), W0)


def _add(net, dev, b):
    net.tower_train_add(_t(b[0], dev), _t(b[1], dev), _t(b[2], dev), _t(b[3], dev))


def _capture(net, c, parts):
    """what the last step saved, as the reference takes it -> dict"""
    B, k, c5 = sum(len(p[3]) for p in parts), c["k"], c["c5"]
    kcat = [T["total_feat"] for T in net._towers]
    xs = [net.debug_tensor("tower_train_x.%d" % t, (B, kc, PP)).cpu().numpy() for t, kc in enumerate(kcat)]
    am = {r: net.debug_tensor("tower_train_argmax.%d" % r, (B, c5, PP)).cpu().numpy().astype(np.int64) for r in sorted(set(REGIONS))}
    acts, row0, images = [], 0, []
    n_conv = len(net._cout)
    for i, p in enumerate(parts):
        maps = []
        for j in range(k + 1):
            l = n_conv - k + j - 1
            ch = net._cout[l]
            hh, ww = P2.map_size(c["cfg"], max(l, n_conv - k))   # (map 0 is the first trained layer's input: its own size)
            maps.append(net.debug_tensor("tower_train_act.%d.%d" % (i, j), (ch, hh, ww)).cpu().numpy())
        n = len(p[3])
        fov = P2.foveal(P2.project(p[1]))
        images.append((maps[0], [m > 0 for m in maps[1:]], {r: am[r][row0:row0 + n] for r in am}, fov))
        acts.append(maps)
        row0 += n
    return dict(xs=xs, am=am, acts=acts, images=images, rest=[x[:, c5:] for x in xs], B=B)


def _judge(tag, r, r64, r32, w_new=None):
    r, r64, r32 = np.asarray(r, np.float64), np.asarray(r64, np.float64), np.asarray(r32, np.float64)
    assert np.isfinite(r).all(), tag
    e = np.abs(r - r64)
    if w_new is not None:
        e = np.maximum(e - U * np.abs(np.asarray(w_new, np.float64)), 0.0)
    y = np.abs(r32 - r64)
    em, er, ym, yr = float(e.max()), float(np.sqrt((e * e).mean())), float(y.max()), float(np.sqrt((y * y).mean()))
    print("ACC %-30s max e %.3g / torch-fp32 %.3g = %.2f   rms e %.3g / %.3g = %.2f" %
          (tag, em, ym, em / ym if ym else (0.0 if em == 0 else np.inf), er, yr, er / yr if yr else (0.0 if er == 0 else np.inf)))
    return em <= MARGIN * ym and er <= MARGIN * yr, (tag, em, ym, er, yr)


def _trainers(W0, c, momentum, wd, lr, norm=True):
    conv = {l: (W0["conv_w.%d" % l], W0["conv_b.%d" % l]) for l in c["layers"]}
    mk = lambda dt: P2.Trainer(W0, conv, c["K"], momentum, wd, mean=MEAN, std=STD, dtype=dt, lr=lr, norm=norm, scale=SCALE)
    return mk(torch.float64), mk(torch.float32)


def _names(c):
    return TT.names(NT) + P2.conv_names(c["layers"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. one step at momentum 0, wd 0, lr 1: the argmax, the Normalize backward, the gradient map, every tensor's gradient
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,case,norm", [("C", "B70_two_images", True), ("C", "B128_one_image", True), ("C", "B1", True),
                                            ("B", "B70_two_images", True), ("C", "B70_two_images", False)])
def test_gradient_against_float64(dev, name, case, norm):
    c = NETS[name]
    P = dict(P2.params(name), conv345_norm=norm)
    net = _net(P, name)
    W0 = _weights(net)
    _stale(net, dev, c, c["k"], momentum=0.0, weight_decay=0.0, bbox_weight=1.0)
    parts = P2.grad_parts(name, case)
    for b in parts:
        _add(net, dev, b)
    loss = net.tower_train_step(1.0).cpu().numpy()
    cap = _capture(net, c, parts)
    B, c5 = cap["B"], c["c5"]
    gx = [net.debug_tensor("tower_train_gx5.%d" % t, (B, c5, PP)).cpu().numpy() for t in range(NT)]
    dx = [net.debug_tensor("tower_train_dx5.%d" % t, (B, c5, PP)).cpu().numpy() for t in range(NT)]
    g5 = [net.debug_tensor("tower_train_g5.%d" % i, cap["acts"][i][-1].shape).cpu().numpy() for i in range(len(parts))]
    Wd = _weights(net)
    net.tower_train_end()
    # item 3: the argmax of every region is own_argmax on the device's saved conv5 map, bit for bit; an empty bin and a zero tie are there
    row0, empty, tie = 0, False, False
    for i, p in enumerate(parts):
        n, top = len(p[3]), cap["acts"][i][-1]
        for r in cap["am"]:
            own = TC.own_argmax(top, cap["images"][i][3][:, r], 7, 7, SCALE)
            assert (own == cap["am"][r][row0:row0 + n]).all(), (i, r)
            empty = empty or bool((own < 0).any())
            if not tie:
                tie = P2.has_zero_tie(top, cap["images"][i][3][:, r], own, SCALE)
        row0 += n
    if B > 1:
        assert empty and tie
    # item 2: dx5 against float64 within the bound the stated order gives (x = the map's values at the argmax, y = the stored operand)
    for t, r in enumerate(REGIONS):
        if not norm:
            assert _bits(dx[t], gx[t])
            continue
        x, row0 = [], 0
        for i, p in enumerate(parts):
            n = len(p[3])
            x.append(TC.gather_pool(torch.from_numpy(cap["acts"][i][-1]), cap["am"][r][row0:row0 + n]).numpy())
            row0 += n
        x, y = np.concatenate(x), cap["xs"][t][:, :c5]
        err = np.abs(dx[t].astype(np.float64) - P2.normalize_backward64(x, y, gx[t]))
        bound = P2.normalize_backward_bound(x, y, gx[t])
        print("ACC %s %s dx5.%d max err / bound %.3f" % (name, case, t, float((err / np.maximum(bound, 1e-300)).max())))
        assert (err <= bound).all(), (t, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.abs(dx[t]).max() > 0
    # item 4: the gradient map is the fp32 chain fed the device's dx5 and argmax, bit for bit; the halo-free interior is all there is
    row0 = 0
    for i, p in enumerate(parts):
        n = len(p[3])
        assert _bits(g5[i], P2.g5_chain(dx, cap["am"], REGIONS, row0, n, cap["acts"][i][-1])), i
        assert np.abs(g5[i]).max() > 0
        row0 += n
    # every tensor's gradient under the yardstick rule
    rois, gt, labels = (np.concatenate([p[j] for p in parts]) for j in (1, 2, 3))
    t64, t32 = _trainers(W0, c, 0.0, 0.0, 1.0, norm)
    l64, G64 = t64.step(cap["images"], REGIONS, cap["rest"], rois, gt, labels, 1.0)
    l32, _ = t32.step(cap["images"], REGIONS, cap["rest"], rois, gt, labels, 1.0)
    P64, P32 = t64.params(), t32.params()
    bad = []
    for n in _names(c):
        w_old = W0[n].astype(np.float64)
        g64 = w_old - P64[n]
        sel = g64[:c["C"]] if (n == "cls_w" and c["K"] > 1) else g64
        assert np.sqrt((sel * sel).mean()) > 0, "%s: the float64 gradient is zero, the case checks nothing" % n
        ok, info = _judge("%s %s%s %s" % (name, case, "" if norm else " unnorm", n), w_old - Wd[n], g64, w_old - P32[n], w_new=Wd[n])
        if not ok:
            bad.append(info)
    ok, info = _judge("%s %s loss" % (name, case), loss, np.array(l64), np.array(l32, np.float32), w_new=loss)
    if not ok:
        bad.append(info)
    for l in range(len(net._cout)):   # a layer that is not trained keeps its bits
        if l not in c["layers"]:
            assert _bits(Wd["conv_w.%d" % l], W0["conv_w.%d" % l]) and _bits(Wd["conv_b.%d" % l], W0["conv_b.%d" % l])
    assert not bad, bad


def test_last_layer_of_44_channels_is_refused(dev):
    """Network D (a last conv layer of 44 channels, K = 1) was to run through test_gradient_against_float64 at B70_two_images.  No
    handle is made for such a trunk: creation refuses feat_c % 8 != 0, before any training state exists.  So the driver never runs
    the Normalize backward, the gather or the mix layer's input gradient with a pad lane in the conv5 slab; their C % 8 != 0 cases in
    tests/test_gpu_train_phase2_kernels_numerics.py check the kernels' own contract."""
    from multipathnet_amd._lib import MpnError
    assert NETS["D"]["c5"] == 44 and NETS["D"]["cfg"][-1] == 44 and NETS["D"]["K"] == 1
    with pytest.raises(MpnError) as e:
        _net(P2.params("D"), "D")
    assert "mpn_mpnet_create" in str(e.value) and "invalid argument: p->feat_c % 8 == 0" in str(e.value), str(e.value)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. three SGD steps (momentum 0.9, wd 5e-4): network C with dropout 0.5 and the classifiers alternating 0, 1, 0; network B plain.
#    Then: a second fresh handle gives the same bits; a net rebuilt from the exported weights detects bit-identically; a graph
#    captured before training replays with the new weights
# ---------------------------------------------------------------------------------------------------------------------------------
SEED = 0x5EED5EED5


def _three_steps(net, dev, c, rate, lr=1e-3, capture=True, stale=True):
    if stale:
        _stale(net, dev, c, c["k"], lr0_step=False, momentum=0.9, weight_decay=5e-4, bbox_weight=1.0, dropout=rate, seed=SEED)
    steps, losses = [], []
    for i in range(3):
        parts = [P2.batch(3000 + 2 * i, 40 - 9 * i, c["C"], 8), P2.batch(3001 + 2 * i, 27 - 4 * i, c["C"], 5)]
        k = i % c["K"]
        net.tower_train_set_head(k)
        for b in parts:
            _add(net, dev, b)
        losses.append(net.tower_train_step(lr))
        if capture:
            steps.append((_capture(net, c, parts), parts, k))
    return steps, torch.stack(losses).cpu().numpy()


@pytest.mark.parametrize("name,rate", [("C", 0.5), ("B", 0.0)])
def test_three_sgd_steps_against_float64(dev, name, rate):
    c = NETS[name]
    P = P2.params(name)
    net = _net(P, name)
    W0 = _weights(net)
    net.set_graphs(True)
    rng = np.random.default_rng(7)
    im = _t(rng.random((3, H, W), dtype=np.float32), dev)
    bx = _t(P2.batch(5, 90, c["C"], 0)[1], dev)

    def test_one(n_):
        d, k = n_.test_one_async(im, bx)
        torch.cuda.synchronize()
        return d[: int(k.item())].cpu().numpy().copy()

    for _ in range(4):
        test_one(net)
    s0, _ = net.detect(im, bx)
    s0 = s0.cpu().numpy().copy()
    replays0 = net.graph_stats()[1]
    assert replays0 > 0
    steps, losses = _three_steps(net, dev, c, rate)
    Wd = _weights(net)
    net.tower_train_end()
    t64, t32 = _trainers(W0, c, 0.9, 5e-4, 1e-3)
    l64, l32 = [], []
    for i, (cap, parts, k) in enumerate(steps):
        rois, gt, labels = (np.concatenate([p[j] for p in parts]) for j in (1, 2, 3))
        drop = TT.masks(SEED, i, NT, cap["B"], c["fc"], rate) if rate else None
        l64.append(t64.step(cap["images"], REGIONS, cap["rest"], rois, gt, labels, 1e-3, k=k, drop=drop)[0])
        l32.append(t32.step(cap["images"], REGIONS, cap["rest"], rois, gt, labels, 1e-3, k=k, drop=drop)[0])
    P64, P32 = t64.params(), t32.params()
    bad = []
    for n in _names(c):
        assert np.isfinite(Wd[n]).all() and not _bits(Wd[n], W0[n]), n
        ok, info = _judge("%s 3 steps %s" % (name, n), Wd[n], P64[n], P32[n], w_new=Wd[n])
        if not ok:
            bad.append(info)
    ok, info = _judge("%s 3 steps losses" % name, losses, np.array(l64), np.array(l32, np.float32), w_new=losses)
    if not ok:
        bad.append(info)
    assert not bad, bad
    # detect and the captured graphs read the new weights; a fresh net of the exported weights is the same network
    for _ in range(4):
        r1 = test_one(net)
    assert net.graph_stats()[1] > replays0, "no graph was replayed after training"
    s1, b1 = net.detect(im, bx)
    torch.cuda.synchronize()
    assert not _bits(s1.cpu().numpy(), s0)
    Wt = dict(net.tower_weights())
    Wt.update(net.trunk_weights())
    fresh = _net(Wt, name)
    s2, b2 = fresh.detect(im, bx)
    torch.cuda.synchronize()
    assert _bits(s1.cpu().numpy(), s2.cpu().numpy()) and _bits(b1.cpu().numpy(), b2.cpu().numpy())
    r2 = test_one(fresh)
    assert len(r1) > 0 and _bits(r1, r2), "the replayed graph does not read the trained weights"
    assert not _diff(Wd, _weights(fresh))
    # determinism: a second fresh handle, the same steps
    net2 = _net(P, name)
    _, losses2 = _three_steps(net2, dev, c, rate, capture=False)
    assert _bits(losses, losses2) and not _diff(Wd, _weights(net2))
    net2.tower_train_end()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. conv_layers = 0 is tower_train_begin, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
def test_conv_layers_0_equals_tower_train_begin(dev):
    c = NETS["C"]
    out = []
    for kw in ({}, {"conv_layers": 0}):
        net = _net(P2.params("C"), "C")
        net.tower_train_begin(momentum=0.9, weight_decay=5e-4, dropout=0.5, seed=SEED, **kw)
        _, losses = _three_steps(net, dev, c, 0.5, capture=False, stale=False)
        out.append((losses, _weights(net)))
        with pytest.raises(Exception, match="conv_layers > 0"):
            net.debug_tensor("tower_train_g5.0", (1,))
        net.tower_train_end()
    # through the C entry point itself (the Python wrapper calls mpn_mpnet_train_begin for 0)
    from multipathnet_amd import _lib
    import ctypes as C
    net = _net(P2.params("C"), "C")
    _lib.check(net._lib.mpn_mpnet_train_begin_conv(net._h, 0, C.c_float(0.9), C.c_float(5e-4), C.c_float(1.0)), "mpn_mpnet_train_begin_conv")
    net._dropout = (0.0, SEED)
    net.tower_train_set_dropout(0.5, SEED)
    _, losses = _three_steps(net, dev, c, 0.5, capture=False, stale=False)
    out.append((losses, _weights(net)))
    net.tower_train_end()
    W0 = _weights(_net(P2.params("C"), "C"))
    for o in out[1:]:
        assert _bits(out[0][0], o[0]) and not _diff(out[0][1], o[1])
    assert all(_bits(out[0][1][n], W0[n]) for n in W0 if n.startswith("conv_"))   # the trunk stayed frozen


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. stop after step 2, checkpoint, resume on a new handle: step 3 is the uninterrupted run's, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
def _one_step(net, dev, c, i):
    net.tower_train_set_head(i % c["K"])
    _add(net, dev, P2.batch(4000 + i, 45 - 6 * i, c["C"], 9))
    return net.tower_train_step(1e-3)


def test_resumed_run_gives_the_bits_of_the_uninterrupted_one(dev, tmp_path):
    from multipathnet_amd import train
    c = NETS["C"]
    full = _net(P2.params("C"), "C")
    full.tower_train_begin(momentum=0.9, weight_decay=5e-4, dropout=0.5, seed=SEED, conv_layers=3)
    losses = torch.stack([_one_step(full, dev, c, i) for i in range(3)]).cpu().numpy()
    W_full, S_full = _weights(full), full.tower_train_state()
    full.tower_train_end()
    first = _net(P2.params("C"), "C")
    first.tower_train_begin(momentum=0.9, weight_decay=5e-4, dropout=0.5, seed=SEED, conv_layers=3)
    l01 = torch.stack([_one_step(first, dev, c, i) for i in range(2)]).cpu().numpy()
    assert _bits(l01, losses[:2])
    path = str(tmp_path / "model_2.t7")
    train.save_checkpoint(path, first)
    first.tower_train_end()
    ck = train.load_checkpoint(path)
    assert ck["kind"] == "mpnet" and ck["conv_layers"] == 3 and ck["state"]["step"] == 2
    assert [v is not None for v in ck["state"]["conv_w"]] == [l in c["layers"] for l in range(len(first._cout))]
    second = _net(ck["weights"], "C")
    second.tower_train_begin(momentum=0.9, weight_decay=5e-4, conv_layers=ck["conv_layers"])
    train.resume(second, ck)
    l2 = _one_step(second, dev, c, 2).cpu().numpy()
    W_res, S_res = _weights(second), second.tower_train_state()
    second.tower_train_end()
    assert _bits(l2, losses[2]) and not _diff(W_full, W_res)
    for l in c["layers"]:
        assert _bits(S_full["conv_w"][l].cpu().numpy(), S_res["conv_w"][l].cpu().numpy()) and np.abs(S_res["conv_w"][l].cpu().numpy()).max() > 0
        assert _bits(S_full["conv_b"][l].cpu().numpy(), S_res["conv_b"][l].cpu().numpy())
    # without the conv momentum the tail ends elsewhere: the state matters
    third = _net(ck["weights"], "C")
    third.tower_train_begin(momentum=0.9, weight_decay=5e-4, conv_layers=3)
    st = dict(ck["state"], conv_w=None, conv_b=None)
    train.resume(third, dict(ck, state=st))
    _one_step(third, dev, c, 2)
    assert _diff(W_full, _weights(third))
    third.tower_train_end()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. train_add_sampled with k = 3 gives the bits of train_add of the restated rows
# ---------------------------------------------------------------------------------------------------------------------------------
def test_add_sampled_is_add_of_the_restated_rows(dev):
    from multipathnet_amd import train
    c = NETS["C"]
    rng = np.random.default_rng(11)
    im = rng.random((3, H, W), dtype=np.float32)
    gtb = np.array([[30, 30, 110, 100], [140, 40, 230, 130]], np.float32)
    gtl = np.array([2, 4], np.int32)
    jit = lambda b, s: b + rng.normal(0, s, (60, 4)).astype(np.float32)
    prop = np.concatenate([jit(gtb[0], 6.0), jit(gtb[1], 25.0)]).astype(np.float32)
    prop[:, 2:] = np.maximum(prop[:, 2:], prop[:, :2] + 8)
    prop = np.clip(prop, 0, np.array([W - 1, H - 1, W - 1, H - 1], np.float32)).astype(np.float32)
    smp = train.DeviceRoiSampler(batch_size=48, fg_fraction=0.25, seed=77)
    out = []
    for sampled in (True, False):
        net = _net(P2.params("C"), "C")
        net.tower_train_begin(momentum=0.9, weight_decay=5e-4, conv_layers=3)
        for draw in (0, 1):
            if sampled:
                n_bg, n_fg = net.tower_train_add_sampled(_t(im, dev), prop, gtb, gtl, smp, draw)
                assert n_bg > 0 and n_fg > 0
            else:
                rec = train.attach_proposals_device(prop, gtb, gtl)
                rois, gt, labels = smp.sample(rec, draw)
                net.tower_train_add(_t(im, dev), rois, gt, labels)
        loss = net.tower_train_step(1e-3).cpu().numpy()
        out.append((loss, _weights(net)))
        net.tower_train_end()
    assert _bits(out[0][0], out[1][0]) and not _diff(out[0][1], out[1][1])
    W0 = _weights(_net(P2.params("C"), "C"))
    assert all(not _bits(out[0][1]["conv_w.%d" % l], W0["conv_w.%d" % l]) for l in c["layers"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. refusals: named, and they change nothing
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from multipathnet_amd._lib import MpnError
    c = NETS["C"]
    net = _net(P2.params("C"), "C")
    for k in (4, -1):
        with pytest.raises(MpnError, match=r"K = 3"):
            net.tower_train_begin(conv_layers=k)
    netB = _net(P2.params("B"), "B")
    with pytest.raises(MpnError, match=r"K = 1"):
        netB.tower_train_begin(conv_layers=2)
    with pytest.raises(MpnError, match="not supported|mpn_mpnet"):   # the plain handle's export keeps refusing these handles
        from multipathnet_amd import _lib
        _lib.check(net._lib.mpn_frcnn_get_trunk_weights(net._h, 0, None, None, None), "mpn_frcnn_get_trunk_weights")
    net.tower_train_begin(momentum=0.9, weight_decay=5e-4, conv_layers=2)   # layers 8 and 9
    W0 = _weights(net)
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    from multipathnet_amd import _lib
    from multipathnet_amd.nn import _f, _stream
    with pytest.raises(MpnError, match=r"layers 8 \.\. 9"):
        _lib.check(net._lib.mpn_mpnet_train_get_trunk_state(net._h, 7, _f(z(48, 40, 3, 3)), _f(z(48)), _stream()), "get")
    with pytest.raises(MpnError, match=r"layers 8 \.\. 9"):
        _lib.check(net._lib.mpn_mpnet_train_set_trunk_state(net._h, 7, _f(z(48, 40, 3, 3)), _f(z(48)), _stream()), "set")
    with pytest.raises(MpnError, match="NULL"):
        _lib.check(net._lib.mpn_mpnet_train_set_trunk_state(net._h, 8, _f(z(12, 48, 3, 3)), None, _stream()), "set")
    _lib.check(net._lib.mpn_mpnet_train_get_trunk_state(net._h, 8, None, None, _stream()), "get")   # get: either may be NULL
    b = P2.batch(1, 10, c["C"], 3)
    for _ in range(8):
        _add(net, dev, b)
    with pytest.raises(MpnError, match="MPN_TRAIN_MAX_IMAGES"):
        _add(net, dev, b)   # the ninth image
    with pytest.raises(MpnError, match="pending"):
        _lib.check(net._lib.mpn_mpnet_train_set_trunk_state(net._h, 8, _f(z(12, 48, 3, 3)), _f(z(12)), _stream()), "set")
    net.tower_train_step(0.0)   # the eight images still step
    assert not _diff(_weights(net), W0)   # lr 0: nothing moved
    # a state set comes back bit for bit
    v = torch.from_numpy(np.random.default_rng(3).standard_normal((12, 48, 3, 3)).astype(np.float32)).to(dev)
    vb = torch.from_numpy(np.random.default_rng(4).standard_normal(12).astype(np.float32)).to(dev)
    _lib.check(net._lib.mpn_mpnet_train_set_trunk_state(net._h, 8, _f(v), _f(vb), _stream()), "set")
    S = net.tower_train_state()
    assert _bits(S["conv_w"][8].cpu().numpy(), v.cpu().numpy()) and _bits(S["conv_b"][8].cpu().numpy(), vb.cpu().numpy()) and S["conv_w"][7] is None
    net.tower_train_scale_momentum(0.5)
    S = net.tower_train_state()
    assert _bits(S["conv_w"][8].cpu().numpy(), (v * 0.5).cpu().numpy())
    net.tower_train_end()
