"""Training the ROI head with dropout behind fc6 and fc7 (mpn_frcnn_train_set_dropout; the reference's default, train.lua:53 /
models/vgg.lua:21) and resumable runs (mpn_frcnn_train_get_state / _set_state, train.save_checkpoint); DESIGN.md section 13.6.

The mask is a pure function of (seed, step, layer, row, column) that tests/dropout_np.py restates in numpy, so the device's mask is
checked EXACTLY, and the float64 step and the PyTorch-CPU fp32 yardstick run with the very masks the device used.  Network, batches,
helpers and THE YARDSTICK RULE (MARGIN = 2.0) are tests/test_gpu_train.py's: cfg [8, 16, P, 16, P, 32], 96 x 160 images, max_rois 200,
heads (fc_dim 96, C 7) — NP pads 96 -> 128, the case where the dropout kernel could touch pad columns — and (128, 4).  Every handle first
runs a 200-ROI detect and a 200-row training step at lr 0, so rows >= B of every buffer the dropout kernel works on are stale.

MEASURED on MI355X (ACC lines of this file, largest max-ratio / rms-ratio over all cases of a test): see DESIGN.md section 13.6."""
import numpy as np
import pytest
import torch

import dropout_np as D
import train_np as T
from test_gpu_train import (GRAD_BATCHES, HEADS, MAXR, MEAN, STD, _add, _batch, _bits, _join, _judge, _net, _np, _params, _pooled, _stale, _weights)

pytestmark = pytest.mark.gpu

SEED = 555


def _y(net, which, B, fc):
    return net.debug_tensor("train_y%d" % which, (B, fc)).cpu().numpy()


def _all_weights(net):
    """head and trunk weights as one flat {name: numpy}"""
    out = _weights(net)
    tw = net.trunk_weights()
    for l, (w, b) in enumerate(zip(tw["conv_w"], tw["conv_b"])):
        out["conv_w.%d" % l], out["conv_b.%d" % l] = w.cpu().numpy(), b.cpu().numpy()
    return out


def _state(net):
    """train_state() as one flat {name: numpy or int}, the untrained tensors left out"""
    S = net.train_state()
    torch.cuda.synchronize()
    out = {"step": S["step"]}
    for k in T.TENSORS:
        if S[k] is not None:
            out[k] = S[k].cpu().numpy()
    for l, (w, b) in enumerate(zip(S["conv_w"], S["conv_b"])):
        if w is not None:
            out["conv_w.%d" % l], out["conv_b.%d" % l] = w.cpu().numpy(), b.cpu().numpy()
    return out


def _same(a, b):
    assert sorted(a) == sorted(b), (sorted(a), sorted(b))
    return [k for k in a if not (a[k] == b[k] if isinstance(a[k], int) else _bits(a[k], b[k]))]


def _stale_step(net, dev, C, seed=77):
    """max_rois rows at lr 0: the minibatch's own buffers (fc6's operand, y6, y7, the head) hold stale rows afterwards"""
    b = _batch(seed, MAXR, C, 60)
    _add(net, dev, b)
    return b, net.train_step(0.0)


def _positive(fc, C):
    """parameters whose fc6 / fc7 pre-activations are all positive (biases raised): every zero behind a dropout is a dropped element"""
    P = dict(_params(fc, C))
    P["fc6_b"], P["fc7_b"] = P["fc6_b"] + 16.0, P["fc7_b"] + 256.0
    return P


def _parts(case, fc, C):
    if case == "B1":
        return [tuple(a[1:2] if j else a for j, a in enumerate(_batch(1234, 2, C, 0)))]
    return [_batch(1000 + 17 * i + fc, n, C, n_bg) for i, (n, n_bg) in enumerate(GRAD_BATCHES[case])]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the mask applied is the mask specified, exactly
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", HEADS, ids=["fc%d_C%d" % h for h in HEADS])
@pytest.mark.parametrize("case", list(GRAD_BATCHES))
def test_mask_applied_is_the_mask_specified(dev, head, case):
    fc, C = head
    net = _net(_positive(fc, C))
    _stale(net, dev)
    net.train_begin(depth=2, momentum=0.0, weight_decay=0.0)
    _stale_step(net, dev, C)
    parts = _parts(case, fc, C)     # B = 70 from two images (rows run on across images), 128, 1
    B = sum(len(p[3]) for p in parts)

    def step(rate):
        net.train_set_dropout(rate, SEED)
        s = net.train_state()["step"]
        for p in parts:
            _add(net, dev, p)
        net.train_step(0.0)         # lr 0, no momentum: the weights stay, every step sees the same pre-dropout activations
        return s, _y(net, 6, B, fc), _y(net, 7, B, fc)

    s0, y6_a, y7_a = step(0.0)
    assert s0 == 1 and y6_a.min() > 0 and y7_a.min() > 0
    for rate in (0.5, 0.25):
        s, y6, y7 = step(rate)
        assert s == s0 + (1 if rate == 0.5 else 2)
        keep6, keep7 = D.keep_mask(SEED, s, 0, B, fc, rate), D.keep_mask(SEED, s, 1, B, fc, rate)
        want6 = np.where(keep6, y6_a * D.scale(rate), np.float32(0.0)).astype(np.float32)     # fl(y * s) in fp32, +0.0 where dropped
        if rate == 0.5:
            assert _bits(want6, np.where(keep6, 2 * y6_a, np.float32(0.0)))
        assert _bits(y6, want6), "rate %g: y6 is not where(keep, fl(y6 * s), +0.0)" % rate
        assert ((y7 == 0) == ~keep7).all(), "rate %g: the zero set of y7 is not the dropped set of layer 1" % rate
        assert not np.signbit(y7[~keep7]).any()
        if B > 1:
            assert 0.3 < keep6.mean() < 0.9 and (keep6 != keep7).any()
    net.train_end()


def test_results_do_not_depend_on_stale_rows_and_pad_columns(dev):
    """rows >= B and columns >= N of y6 / y7 are neither read nor written: two handles whose 200-row steps left different values there
    (another batch, another rate, another seed) give the same bits in the steps that follow"""
    fc, C = HEADS[0]    # fc_dim 96: NP = 128, 32 pad columns
    P = _params(fc, C)
    out = []
    for stale_seed, stale_rate, stale_drop_seed in ((77, 0.5, 9), (78, 0.25, 10)):
        net = _net(P)
        _stale(net, dev)
        net.train_begin(depth=2, momentum=0.0, weight_decay=0.0, dropout=stale_rate, seed=stale_drop_seed)
        _stale_step(net, dev, C, seed=stale_seed)
        net.train_set_dropout(0.5, SEED)
        res = []
        for parts in (_parts("B70_two_images", fc, C), [_batch(2001, 53, C, 12)]):
            for p in parts:
                _add(net, dev, p)
            B = sum(len(p[3]) for p in parts)
            res += [net.train_step(1e-2).cpu().numpy(), _y(net, 6, B, fc), _y(net, 7, B, fc)]
        res += list(_weights(net).values())
        net.train_end()
        out.append(res)
    assert not _bits(out[0][1], np.zeros_like(out[0][1]))
    for a, b in zip(*out):
        assert _bits(a, b)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. rate 0 is the code without dropout: the same bits with and without the call
# ---------------------------------------------------------------------------------------------------------------------------------
def _steps(net, dev, C, n, first=0, lr=1e-3, seed0=2000):
    losses = []
    for i in range(first, first + n):
        _add(net, dev, _batch(seed0 + i, 66 - 13 * (i % 4), C, 12))   # shrinking batches: rows >= B hold the previous step's values
        losses.append(net.train_step(lr))
    return torch.stack(losses).cpu().numpy()


@pytest.mark.parametrize("depth", [0, 1, 2, "trunk3"])
def test_rate_zero_is_no_dropout(dev, depth):
    fc, C = HEADS[0]
    P = _params(fc, C)
    kw = {"trunk_layers": 3} if depth == "trunk3" else {"depth": depth}
    runs = []
    for call in (False, True):
        net = _net(P)
        _stale(net, dev)
        net.train_begin(momentum=0.9, weight_decay=5e-4, **kw)
        if call:
            net.train_set_dropout(0.0, 123456789)
        losses = _steps(net, dev, C, 3)
        runs.append((losses, _all_weights(net), _state(net)))
        net.train_end()
    assert runs[0][2]["step"] == 3
    assert _bits(runs[0][0], runs[1][0])
    assert not _same(runs[0][1], runs[1][1]) and not _same(runs[0][2], runs[1][2])


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the gradient and three SGD steps against float64 with the same masks (tests/test_gpu_train.py's yardstick rule, its MARGIN)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", HEADS, ids=["fc%d_C%d" % h for h in HEADS])
@pytest.mark.parametrize("case", list(GRAD_BATCHES))
def test_gradient_against_float64_with_the_same_masks(dev, head, case):
    fc, C = head
    P = _params(fc, C)
    P0 = _np(P)
    net = _net(P)
    _stale(net, dev)
    net.train_begin(depth=2, momentum=0.0, weight_decay=0.0, bbox_weight=1.0, dropout=0.5, seed=SEED)
    _stale_step(net, dev, C)
    assert all(_bits(v, P0[k]) for k, v in _weights(net).items())
    parts = _parts(case, fc, C)
    step = net.train_state()["step"]
    assert step == 1
    for b in parts:
        _add(net, dev, b)
    loss = net.train_step(1.0).cpu().numpy()
    rois, gt, labels = _join(parts)
    B = len(labels)
    x = _pooled(net, B)
    y6 = _y(net, 6, B, fc)
    Wd = _weights(net)
    net.train_end()
    m6, m7 = D.multipliers(SEED, step, B, fc, 0.5)
    assert (y6[m6 == 0] == 0).all() and (y6[m6 > 0] > 0).any()     # the float side's masks are the device's
    ref = D.Sgd64(P0, depth=2, momentum=0.0, weight_decay=0.0, mean=MEAN, std=STD)
    l64, d = ref.step(x, rois, gt, labels, m6, m7, lr=1.0)
    P32, l32 = D.torch_steps(P0, [(x, rois, gt, labels, m6, m7)], 1.0, depth=2, momentum=0.0, weight_decay=0.0, mean=MEAN, std=STD, dtype=torch.float32)
    bad = []
    for k in T.TENSORS:
        w_old = P0[k].astype(np.float64)
        ok, info = _judge("drop %s %s" % (case, k), w_old - Wd[k], w_old - ref.P[k], w_old - P32[k], w_new=Wd[k])
        if not ok:
            bad.append(info)
    ok, info = _judge("drop %s loss" % case, loss, np.array(l64), np.array(l32[0], np.float32), w_new=loss)
    if not ok:
        bad.append(info)
    assert not bad, bad


@pytest.mark.parametrize("head", HEADS, ids=["fc%d_C%d" % h for h in HEADS])
@pytest.mark.parametrize("depth", [0, 1, 2])
def test_three_sgd_steps_against_float64_with_the_same_masks(dev, head, depth):
    """the 200-row step at lr 0 is part of the run on both sides: it moves no weight but leaves its gradient in the momentum"""
    fc, C = head
    P = _params(fc, C)
    P0 = _np(P)
    net = _net(P)
    _stale(net, dev)
    net.train_begin(depth=depth, momentum=0.9, weight_decay=5e-4, bbox_weight=1.0, dropout=0.5, seed=SEED)
    batches, lrs, losses = [], [], []
    for i in range(4):
        b = _batch(77, MAXR, C, 60) if i == 0 else _batch(1999 + i, 66 - 13 * (i - 1), C, 12)
        lrs.append(0.0 if i == 0 else 1e-3)
        step = net.train_state()["step"]
        assert step == i
        _add(net, dev, b)
        losses.append(net.train_step(lrs[-1]))
        n = len(b[3])
        batches.append((_pooled(net, n), b[1], b[2], b[3]) + D.multipliers(SEED, step, n, fc, 0.5))
    losses = torch.stack(losses).cpu().numpy()
    Wd = _weights(net)
    net.train_end()
    ref = D.Sgd64(P0, depth=depth, momentum=0.9, weight_decay=5e-4, mean=MEAN, std=STD)
    l64 = [ref.step(*b, lr=lr)[0] for b, lr in zip(batches, lrs)]
    P32, l32 = D.torch_steps(P0, batches, lrs, depth=depth, momentum=0.9, weight_decay=5e-4, mean=MEAN, std=STD, dtype=torch.float32)
    bad = []
    for k in T.TENSORS:
        if k not in T.TRAINED[depth]:
            assert _bits(Wd[k], P0[k]), "%s is outside depth %d and changed" % (k, depth)
            continue
        assert np.isfinite(Wd[k]).all() and not _bits(Wd[k], P0[k]), k
        ok, info = _judge("drop depth%d %s" % (depth, k), Wd[k], ref.P[k], P32[k], w_new=Wd[k])
        if not ok:
            bad.append(info)
    ok, info = _judge("drop depth%d losses" % depth, losses, np.array(l64), np.array(l32, np.float32), w_new=losses)
    if not ok:
        bad.append(info)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the stream: seed and step decide the masks, nothing else does; inference never sees dropout
# ---------------------------------------------------------------------------------------------------------------------------------
def test_stream_is_seed_and_step(dev):
    fc, C = HEADS[0]
    P = _params(fc, C)
    runs = []
    for seed in (SEED, SEED, SEED + 1, SEED + (1 << 32)):     # (the last differs in the key's high word alone)
        net = _net(P)
        _stale(net, dev)
        net.train_begin(depth=2, momentum=0.9, weight_decay=5e-4, dropout=0.5, seed=seed)
        losses = _steps(net, dev, C, 3)
        runs.append((losses, _weights(net)))
        net.train_end()
    assert _bits(runs[0][0], runs[1][0]) and all(_bits(runs[0][1][k], runs[1][1][k]) for k in T.TENSORS)
    for other in runs[2:]:
        assert not _bits(runs[0][0], other[0]) and all(not _bits(runs[0][1][k], other[1][k]) for k in ("fc6_w", "fc7_w", "cls_w", "bbox_w"))


def test_consecutive_steps_use_different_masks_and_detect_sees_none(dev):
    fc, C = HEADS[0]
    net = _net(_positive(fc, C))
    im, bx, s0, b0 = _stale(net, dev)
    net.train_begin(depth=2, momentum=0.0, weight_decay=0.0, dropout=0.5, seed=SEED)
    b = _batch(2000, 66, C, 12)
    zero = []
    for step in (0, 1):
        assert net.train_state()["step"] == step
        _add(net, dev, b)
        net.train_step(0.0)
        zero.append(_y(net, 6, 66, fc) == 0)
        assert (zero[-1] == ~D.keep_mask(SEED, step, 0, 66, fc, 0.5)).all(), step
        s1, b1 = net.detect(im, bx)     # between steps, at lr 0: the bits of before training began
        assert _bits(s0.cpu().numpy(), s1.cpu().numpy()) and _bits(b0.cpu().numpy(), b1.cpu().numpy())
    assert (zero[0] != zero[1]).any() and (zero[0] != ~D.keep_mask(SEED, 1, 0, 66, fc, 0.5)).any()
    net.train_end()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. resume, bit for bit: two steps, state + weights out, a new handle from them, two more steps == four steps straight
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [2, "trunk3"])
def test_resume_bit_for_bit(dev, depth, tmp_path):
    from multipathnet_amd import train
    fc, C = HEADS[0]
    P = _params(fc, C)
    kw = dict(momentum=0.9, weight_decay=5e-4)
    kw.update({"trunk_layers": 3} if depth == "trunk3" else {"depth": depth})
    a = _net(P)
    _stale(a, dev)
    a.train_begin(dropout=0.5, seed=SEED, **kw)
    losses_a = _steps(a, dev, C, 4)
    Wa, Sa = _all_weights(a), _state(a)
    a.train_end()

    b = _net(P)
    _stale(b, dev)
    b.train_begin(dropout=0.5, seed=SEED, **kw)
    losses_b = [_steps(b, dev, C, 2)]
    Pn = dict(P)
    if depth == 2:     # through one .t7 file
        path = str(tmp_path / "ckpt_2.t7")
        train.save_checkpoint(path, b)
        b.train_end()
        ck = train.load_checkpoint(path)
        assert ck["dropout"] == 0.5 and ck["seed"] == SEED and ck["state"]["step"] == 2
        assert ck["state"]["conv_w"] == [None] * 4 and ck["state"]["fc6_w"] is not None
        Pn.update(ck["weights"])
        c = _net(Pn)
        _stale(c, dev)
        c.train_begin(**kw)
        train.resume(c, ck)
    else:
        S, Wh, Wt = b.train_state(), b.head_weights(), b.trunk_weights()
        torch.cuda.synchronize()
        assert S["step"] == 2 and S["conv_w"][0] is None and all(S["conv_w"][l] is not None for l in (1, 2, 3))
        S = {k: ([None if t is None else t.cpu() for t in v] if isinstance(v, list) else (v if isinstance(v, int) or v is None else v.cpu())) for k, v in S.items()}
        b.train_end()
        Pn.update({k: v.cpu() for k, v in Wh.items()})
        Pn["conv_w"], Pn["conv_b"] = [w.cpu() for w in Wt["conv_w"]], [w.cpu() for w in Wt["conv_b"]]
        c = _net(Pn)
        _stale(c, dev)
        c.train_begin(**kw)
        c.train_set_dropout(0.5, SEED)
        c.train_load_state(S)
    assert c.train_state()["step"] == 2
    losses_b.append(_steps(c, dev, C, 2, first=2))
    Wc, Sc = _all_weights(c), _state(c)
    c.train_end()
    assert _bits(losses_a, np.concatenate(losses_b))
    assert not _same(Wa, Wc), _same(Wa, Wc)
    assert Sc["step"] == 4 and not _same(Sa, Sc), _same(Sa, Sc)
    assert not _bits(Wa["fc6_w"], _np(P)["fc6_w"])


def test_state_round_trip_is_exact(dev):
    """get -> set -> get returns the same bits (momentum of an odd-sized head: 5C = 35 rows in 128, K = 96 in 128)"""
    fc, C = HEADS[0]
    net = _net(_params(fc, C))
    _stale(net, dev)
    net.train_begin(trunk_layers=3, momentum=0.9, weight_decay=5e-4, dropout=0.5, seed=SEED)
    _steps(net, dev, C, 2)
    S1, flat1 = net.train_state(), _state(net)
    assert all(np.abs(flat1[k]).max() > 0 for k in flat1 if k != "step")
    S1["step"] = 41
    net.train_load_state(S1)
    flat2 = _state(net)
    assert flat2.pop("step") == 41 and flat1.pop("step") == 2
    assert not _same(flat1, flat2)
    net.train_end()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    import ctypes as C_
    from multipathnet_amd import MpnError
    from multipathnet_amd.nn import _f, _stream
    fc, C = HEADS[1]
    net = _net(_params(fc, C))
    _stale(net, dev)
    for call in (lambda: net.train_set_dropout(0.5, 1), lambda: net.train_state()):     # no train_begin
        with pytest.raises(MpnError) as ei:
            call()
        assert "status -5" in str(ei.value) and "no mpn_frcnn_train_begin" in str(ei.value)
    net.train_begin(depth=1)
    for rate in (1.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(MpnError) as ei:
            net.train_set_dropout(rate, 1)
        assert "status -1" in str(ei.value) and "rate" in str(ei.value)
    S = net.train_state()
    assert S["fc6_w"] is None and S["fc6_b"] is None and S["fc7_w"] is not None and S["conv_w"] == [None] * 4
    # a tensor the depth does not train has no momentum: a non-NULL pointer is refused, naming it
    z = torch.zeros(fc * 32 * 49, dtype=torch.float32, device=dev)
    lib, step = net._lib, C_.c_long()
    rc = lib.mpn_frcnn_train_get_state(net._h, _f(z), None, None, None, None, None, None, None, C_.byref(step), _stream())
    assert rc == -1 and b"d_fc6_v " in lib.mpn_last_error()
    rc = lib.mpn_frcnn_train_set_state(net._h, None, _f(z), _f(S["fc7_w"]), _f(S["fc7_b"]), _f(S["cls_w"]), _f(S["cls_b"]), _f(S["bbox_w"]), _f(S["bbox_b"]), 0, _stream())
    assert rc == -1 and b"d_fc6_vb " in lib.mpn_last_error()
    # ... and a trained one that is missing from set_state
    rc = lib.mpn_frcnn_train_set_state(net._h, None, None, _f(S["fc7_w"]), None, _f(S["cls_w"]), _f(S["cls_b"]), _f(S["bbox_w"]), _f(S["bbox_b"]), 0, _stream())
    assert rc == -1 and b"d_fc7_vb " in lib.mpn_last_error()
    rc = lib.mpn_frcnn_train_set_state(net._h, None, None, _f(S["fc7_w"]), _f(S["fc7_b"]), _f(S["cls_w"]), _f(S["cls_b"]), _f(S["bbox_w"]), _f(S["bbox_b"]), -1, _stream())
    assert rc == -1 and b"step" in lib.mpn_last_error()
    for l in (0, 3, 4, -1):     # depth 1 trains no conv layer
        for fn in (lib.mpn_frcnn_train_get_trunk_state, lib.mpn_frcnn_train_set_trunk_state):
            assert fn(net._h, l, _f(z), _f(z), _stream()) == -1 and b"conv layer" in lib.mpn_last_error()
    # rows pending: the state cannot be replaced under them
    _add(net, dev, _batch(8000, 20, C, 5))
    with pytest.raises(MpnError) as ei:
        net.train_load_state(S)
    assert "status -5" in str(ei.value) and "pending" in str(ei.value)
    net.train_set_dropout(0.5, 3)     # (allowed with rows pending: it takes effect at the next step)
    net.train_step(1e-3)
    net.train_load_state(S)
    net.train_end()
    net.train_begin(trunk_layers=2)
    assert lib.mpn_frcnn_train_get_trunk_state(net._h, 1, _f(z), _f(z), _stream()) == -1 and b"layers 2 .. 3" in lib.mpn_last_error()
    _add(net, dev, _batch(8001, 20, C, 5))
    assert lib.mpn_frcnn_train_set_trunk_state(net._h, 3, _f(z), _f(z), _stream()) == -5 and b"pending" in lib.mpn_last_error()
    assert lib.mpn_frcnn_train_get_trunk_state(net._h, 3, _f(z), _f(z), _stream()) == 0
    net.train_step(0.0)
    assert lib.mpn_frcnn_train_set_trunk_state(net._h, 3, _f(z), None, _stream()) == -1 and b"d_vb" in lib.mpn_last_error()
    net.train_end()
    with pytest.raises(MpnError):
        net.train_set_dropout(0.5, 1)
