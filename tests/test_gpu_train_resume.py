"""Resumable tower training on the device: the optimiser state of a MultiPathNet handle out and in
(mpn_mpnet_train_get_state / _set_state / _get_head_state / _set_head_state), the learning-rate drop on the momentum
(mpn_frcnn_train_scale_momentum / mpn_mpnet_train_scale_momentum), checkpoints of a tower run and train.fit's epoch loop.

Everything here is bit for bit except test 3, whose bound is derived below.  The networks are the training tests' own:
  towers  A and B of tests/test_gpu_train_towers.py (150 x 250 images, max_rois 200, five towers); B has Kcat 112 -> 128, c5 48 -> 128,
          K*C = 7: every packed buffer has pad lanes and odd widths
  plain   tests/test_gpu_train_trunk.py's six-layer VGG shape at MPN_TRAIN_TRUNK(3) (fc6, fc7, heads and three conv layers trained)
Every buffer the state is exported into lies between NaN guard zones and is pre-filled with NaN: a write outside it, or an element the
export skips, shows.

3. THE BOUND.  sgd_wgrad_kernel (and its segmented and bias forms) ends with  v = momentum * v + g';  w = w - lr * v,  each operation
rounded on its own (train.h), and stores that v.  With lr = 2^-10 the product lr * v is exact in fp32 (a power of two; the values
are far from the subnormal range), so w_new = fl(w_old - lr * v) carries ONE rounding, that of the subtraction: at most half an ulp of
w_new, i.e. |(w_old - w_new) - lr * v| <= 2^-24 |w_new|, evaluated in float64 where w_old - w_new and lr * v are exact.  A fused
multiply-subtract would round once as well, so the bound does not depend on contraction."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_sampler as GS  # noqa: E402
import test_gpu_train_towers as G  # noqa: E402
import test_gpu_train_trunk as TR  # noqa: E402
import train_towers_np as TT  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
TOWER = ("mix_w", "mix_b", "fc6_w", "fc6_b", "fc7_w", "fc7_b")
HEADS = ("cls_w", "cls_b", "bbox_w", "bbox_b")
PLAIN = ("fc6_w", "fc6_b", "fc7_w", "fc7_b", "cls_w", "cls_b", "bbox_w", "bbox_b")
PLAIN_FC, PLAIN_C, PLAIN_CONVS = 96, 7, (3, 4, 5)   # the plain network; the layers MPN_TRAIN_TRUNK(3) trains
SEED64 = 0x7EDCBA9876543210
EINVAL, ESTATE = -1, -5
_t, _bits = G._t, G._bits


def _lib_calls():
    from multipathnet_amd import _lib
    from multipathnet_amd.nn import _f, _stream
    return _lib, _f, _stream


def _guarded(dev, shape):
    n = int(np.prod(shape))
    full = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
    return full, full[GUARD:GUARD + n].view(*shape)


def _collect(bufs):
    """the exported tensors as numpy; the guard zones still NaN, every element of every buffer written"""
    torch.cuda.synchronize()
    out = {}
    for n, (full, view) in bufs.items():
        h = full.cpu().numpy()
        assert np.isnan(h[:GUARD]).all() and np.isnan(h[-GUARD:]).all(), "%s: a guard zone was written" % n
        assert not np.isnan(h[GUARD:-GUARD]).any(), "%s: an element was not written" % n
        out[n] = h[GUARD:-GUARD].reshape(tuple(view.shape)).copy()
    return out


# ---- the towers' state, flat under train_towers_np's names ("t<t>.<name>", the four heads) + "step" ----
def _tower_shapes(net):
    F, Cn, KC = net.fc_dim, net.n_classes, net.n_integral * net.n_classes
    c5, nf = net._cout[-1], len(net._towers) - 1
    sh = {}
    for t, T in enumerate(net._towers):
        sh.update({"t%d.mix_w" % t: (c5, T["total_feat"]), "t%d.mix_b" % t: (c5,), "t%d.fc6_w" % t: (F, c5 * G.PP), "t%d.fc6_b" % t: (F,),
                   "t%d.fc7_w" % t: (F, F), "t%d.fc7_b" % t: (F,)})
    sh.update(cls_w=(KC, nf * F), cls_b=(KC,), bbox_w=(4 * Cn, F), bbox_b=(4 * Cn,))
    return sh


def _tower_state(net, dev):
    _lib, _f, _stream = _lib_calls()
    bufs = {n: _guarded(dev, s) for n, s in _tower_shapes(net).items()}
    for t in range(len(net._towers)):
        _lib.check(net._lib.mpn_mpnet_train_get_state(net._h, t, *[_f(bufs["t%d.%s" % (t, k)][1]) for k in TOWER], _stream()), "get_state")
    step = C.c_long(-1)
    _lib.check(net._lib.mpn_mpnet_train_get_head_state(net._h, *[_f(bufs[k][1]) for k in HEADS], C.byref(step), _stream()), "get_head_state")
    out = _collect(bufs)
    out["step"] = int(step.value)
    return out


def _structured(S):
    out = {"towers": [{k: S["t%d.%s" % (t, k)] for k in TOWER} for t in range(G.NT)], "step": S["step"]}
    out.update({k: S[k] for k in HEADS})
    return out


def _tower_weights(net):
    torch.cuda.synchronize()
    return TT.flat(net.tower_weights())


# ---- the plain handle's, under "fc6_w" .. "bbox_b", "conv_w.<l>", "conv_b.<l>" + "step" ----
def _plain_net():
    return TR._net(TR._params(PLAIN_FC, PLAIN_C))


def _plain_state(net, dev):
    _lib, _f, _stream = _lib_calls()
    F, Cn = PLAIN_FC, PLAIN_C
    sh = {"fc6_w": (F, TR.K6), "fc6_b": (F,), "fc7_w": (F, F), "fc7_b": (F,), "cls_w": (Cn, F), "cls_b": (Cn,), "bbox_w": (4 * Cn, F), "bbox_b": (4 * Cn,)}
    for l in PLAIN_CONVS:
        sh["conv_w.%d" % l], sh["conv_b.%d" % l] = (TR.COUT[l], TR.COUT[l - 1], 3, 3), (TR.COUT[l],)
    bufs = {n: _guarded(dev, s) for n, s in sh.items()}
    step = C.c_long(-1)
    _lib.check(net._lib.mpn_frcnn_train_get_state(net._h, *[_f(bufs[k][1]) for k in PLAIN], C.byref(step), _stream()), "get_state")
    for l in PLAIN_CONVS:
        _lib.check(net._lib.mpn_frcnn_train_get_trunk_state(net._h, l, _f(bufs["conv_w.%d" % l][1]), _f(bufs["conv_b.%d" % l][1]), _stream()), "trunk")
    out = _collect(bufs)
    out["step"] = int(step.value)
    return out


def _plain_structured(S):
    out = {k: S[k] for k in PLAIN}
    out["conv_w"] = [S.get("conv_w.%d" % l) for l in range(TR.NL)]
    out["conv_b"] = [S.get("conv_b.%d" % l) for l in range(TR.NL)]
    out["step"] = S["step"]
    return out


def _plain_weights(net):
    W = TR._weights(net)
    out = {k: W[k] for k in PLAIN}
    for l in range(TR.NL):
        out["conv_w.%d" % l], out["conv_b.%d" % l] = W["conv_w"][l], W["conv_b"][l]
    return out


def _random_state(S0, seed):
    """values of S0's shapes with -0.0, subnormals and the smallest normal number among them"""
    rng = np.random.default_rng(seed)
    special = np.array([-0.0, 1e-42, -3e-45, 1.1754944e-38, -2e-39], np.float32)
    out = {}
    for n, a in S0.items():
        if n == "step":
            continue
        v = (rng.standard_normal(a.shape) * 0.01).astype(np.float32)
        v.reshape(-1)[:special.size] = special[:v.size]
        out[n] = v
    out["step"] = 41
    return out


def _scaled(S, f):
    out = {n: (np.float32(f) * a if n != "step" else a) for n, a in S.items()}
    assert all(a.dtype == np.float32 for n, a in out.items() if n != "step")
    return out


def _diff(Sa, Sb):
    """the names whose bits differ"""
    assert set(Sa) == set(Sb)
    return [n for n in Sa if (Sa[n] != Sb[n] if n == "step" else not _bits(Sa[n], Sb[n]))]


def _tower_step(net, dev, c, i, lr=1e-3):
    """step i of a run: two images, the integral head alternating"""
    net.tower_train_set_head(i % c["K"])
    for j in range(2):
        G._add(net, dev, G._batch(3000 + 10 * i + j, 34 + 7 * j - 3 * i, c["C"], 8))
    return net.tower_train_step(lr)


def _plain_step(net, dev, i, lr=1e-3):
    for j in range(2):
        TR._add(net, dev, TR._batch(3100 + 10 * i + j, 30 + 5 * j, PLAIN_C, 8, TR.SIZES[j]))
    return net.train_step(lr)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. fresh state   2. round trip
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.CONFIGS))
def test_fresh_state_is_zero_and_a_set_state_comes_back_bit_for_bit(dev, name):
    net = G._net(G._params(name), name)
    net.tower_train_begin()
    S0 = _tower_state(net, dev)
    assert S0["step"] == 0
    for n, a in S0.items():
        if n != "step":
            assert (a.view(np.uint32) == 0).all(), "%s: the momentum after begin is not +0.0 everywhere" % n
    R = _random_state(S0, 5)
    assert any(np.signbit(a).any() and (a == 0).any() for n, a in R.items() if n != "step")   # a -0.0 is among the values
    net.tower_train_load_state(_structured(R))
    S1 = _tower_state(net, dev)
    assert not _diff(S1, R)
    # the Python method returns the same tensors
    Sp = net.tower_train_state()
    torch.cuda.synchronize()
    assert Sp["step"] == 41 and len(Sp["towers"]) == G.NT
    assert all(_bits(Sp["towers"][t][k].cpu().numpy(), R["t%d.%s" % (t, k)]) for t in range(G.NT) for k in TOWER)
    assert all(_bits(Sp[k].cpu().numpy(), R[k]) for k in HEADS)
    net.tower_train_end()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the exported momentum is the one the update used
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.CONFIGS))
def test_exported_momentum_is_what_the_update_used(dev, name):
    c = G.CONFIGS[name]
    net = G._net(G._params(name), name)
    net.tower_train_begin(momentum=0.9, weight_decay=5e-4)
    _tower_step(net, dev, c, 0)   # the state is no longer zero, no weight is exactly zero
    W_old = _tower_weights(net)
    lr = 2.0 ** -10
    _tower_step(net, dev, c, 1, lr=lr)
    W_new, V = _tower_weights(net), _tower_state(net, dev)
    net.tower_train_end()
    assert V["step"] == 2
    bad = []
    for n in TT.names(G.NT):
        v, w0, w1 = V[n].astype(np.float64), W_old[n].astype(np.float64), W_new[n].astype(np.float64)
        assert np.abs(v).max() > 0 and not _bits(W_old[n], W_new[n]), n
        assert np.abs(V[n][V[n] != 0]).min() > 2.0 ** -116, n   # lr * v is a normal number: the product is exact
        err = np.abs((w0 - w1) - lr * v) - 2.0 ** -24 * np.abs(w1)
        print("STATE %s %-10s max(|dw - lr v| - 2^-24 |w|) = %.3g" % (name, n, err.max()))
        if err.max() > 0:
            bad.append((n, float(err.max())))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. resume is exact
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rate", [("A", 0.5), ("B", 0.0)])
def test_resumed_tower_run_gives_the_bits_of_the_uninterrupted_one(dev, tmp_path, name, rate):
    from multipathnet_amd import train
    c = G.CONFIGS[name]
    full = G._net(G._params(name), name)
    full.tower_train_begin(momentum=0.9, weight_decay=5e-4, dropout=rate, seed=SEED64)
    losses = torch.stack([_tower_step(full, dev, c, i) for i in range(4)]).cpu().numpy()
    W_full, S_full = _tower_weights(full), _tower_state(full, dev)
    full.tower_train_end()

    first = G._net(G._params(name), name)
    first.tower_train_begin(momentum=0.9, weight_decay=5e-4, dropout=rate, seed=SEED64)
    l01 = torch.stack([_tower_step(first, dev, c, i) for i in range(2)]).cpu().numpy()
    assert _bits(l01, losses[:2])
    path = str(tmp_path / "model_2.t7")
    train.save_checkpoint(path, first)
    first.tower_train_end()
    first.close()
    del first

    ck = train.load_checkpoint(path)
    assert ck["kind"] == "mpnet" and ck["seed"] == SEED64 and ck["dropout"] == rate and ck["state"]["step"] == 2
    second = G._net(ck["weights"], name)
    assert second.is_mpnet and second.n_integral == c["K"]
    second.tower_train_begin(momentum=0.9, weight_decay=5e-4)
    train.resume(second, ck)
    l23 = torch.stack([_tower_step(second, dev, c, i) for i in (2, 3)]).cpu().numpy()
    W_res, S_res = _tower_weights(second), _tower_state(second, dev)
    second.tower_train_end()
    assert _bits(l23, losses[2:])
    assert not G._all_bits(W_full, W_res)
    assert not _diff(S_full, S_res) and S_res["step"] == 4
    if rate:   # the dropout stream matters: the same tail under another seed ends elsewhere
        other = G._net(ck["weights"], name)
        other.tower_train_begin(momentum=0.9, weight_decay=5e-4)
        train.resume(other, dict(ck, seed=SEED64 ^ 1))
        lo = torch.stack([_tower_step(other, dev, c, i) for i in (2, 3)]).cpu().numpy()
        other.tower_train_end()
        assert not _bits(lo, losses[2:])


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. scaling
# ---------------------------------------------------------------------------------------------------------------------------------
def _scale_sweep(get, load, scale, S0):
    R = _random_state(S0, 9)
    load(R)
    cur = R
    for f in (0.1, 0.5, 1.0, 0.0):
        scale(f)
        want = _scaled(cur, f)
        if f == 1.0:
            assert not _diff(want, cur)
        got = get()
        assert not _diff(got, want), (f, _diff(got, want))
        cur = got
    assert all((a == 0).all() for n, a in cur.items() if n != "step") and cur["step"] == 41   # (a -0.0 times 0.0f stays -0.0)


@pytest.mark.parametrize("name", list(G.CONFIGS))
def test_tower_scale_momentum_is_one_fp32_multiply(dev, name):
    c = G.CONFIGS[name]
    a, b = G._net(G._params(name), name), G._net(G._params(name), name)
    a.tower_train_begin(momentum=0.9, weight_decay=5e-4)
    b.tower_train_begin(momentum=0.9, weight_decay=5e-4)
    _scale_sweep(lambda: _tower_state(a, dev), lambda S: a.tower_train_load_state(_structured(S)), a.tower_train_scale_momentum, _tower_state(a, dev))
    # what the next update reads in the packed layout: a twin whose state was replaced through set_state with the numpy-scaled tensors
    zero = {n: (np.zeros_like(v) if n != "step" else 0) for n, v in _tower_state(a, dev).items()}
    a.tower_train_load_state(_structured(zero))
    la, lb = _tower_step(a, dev, c, 0), _tower_step(b, dev, c, 0)
    assert _bits(la.cpu().numpy(), lb.cpu().numpy()) and not _diff(_tower_state(a, dev), _tower_state(b, dev))
    a.tower_train_scale_momentum(0.1)
    b.tower_train_load_state(_structured(_scaled(_tower_state(b, dev), 0.1)))
    la, lb = _tower_step(a, dev, c, 1), _tower_step(b, dev, c, 1)
    assert _bits(la.cpu().numpy(), lb.cpu().numpy())
    assert not G._all_bits(_tower_weights(a), _tower_weights(b))
    Sa = _tower_state(a, dev)
    assert not _diff(Sa, _tower_state(b, dev)) and Sa["step"] == 2
    a.tower_train_end()
    b.tower_train_end()


def test_plain_scale_momentum_covers_fc_heads_and_the_trained_conv_layers(dev):
    a, b = _plain_net(), _plain_net()
    a.train_begin(trunk_layers=3, momentum=0.9, weight_decay=5e-4)
    b.train_begin(trunk_layers=3, momentum=0.9, weight_decay=5e-4)
    S0 = _plain_state(a, dev)
    assert S0["step"] == 0 and {"conv_w.3", "conv_b.4", "conv_w.5", "fc6_w", "bbox_b"} <= set(S0)
    _scale_sweep(lambda: _plain_state(a, dev), lambda S: a.train_load_state(_plain_structured(S)), a.train_scale_momentum, S0)
    zero = {n: (np.zeros_like(v) if n != "step" else 0) for n, v in S0.items()}
    a.train_load_state(_plain_structured(zero))
    _plain_step(a, dev, 0), _plain_step(b, dev, 0)
    assert not _diff(_plain_state(a, dev), _plain_state(b, dev))
    a.train_scale_momentum(0.1)
    Sb = _plain_state(b, dev)
    assert all(np.abs(v).max() > 0 for n, v in Sb.items() if n != "step")
    b.train_load_state(_plain_structured(_scaled(Sb, 0.1)))
    la, lb = _plain_step(a, dev, 1), _plain_step(b, dev, 1)
    assert _bits(la.cpu().numpy(), lb.cpu().numpy())
    Wa, Wb = _plain_weights(a), _plain_weights(b)
    assert not [n for n in Wa if not _bits(Wa[n], Wb[n])]
    assert not _diff(_plain_state(a, dev), _plain_state(b, dev))
    a.train_end()
    b.train_end()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def _refused(lib, rc, want_rc, *words):
    msg = lib.mpn_last_error().decode()
    assert rc == want_rc, (rc, want_rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_refusals_are_named_change_nothing_and_leave_the_handle_training(dev):
    _lib, _f, _stream = _lib_calls()
    c = G.CONFIGS["A"]
    net, twin, plain = G._net(G._params("A"), "A"), G._net(G._params("A"), "A"), _plain_net()
    lib, h, s, f = net._lib, net._h, _stream(), C.c_float
    sh = _tower_shapes(net)
    z = {n: torch.zeros(shape, dtype=torch.float32, device=dev) + 0.25 for n, shape in sh.items()}
    tower0 = [_f(z["t0.%s" % k]) for k in TOWER]
    heads = [_f(z[k]) for k in HEADS]
    step = C.c_long(-7)
    # no begin
    _refused(lib, lib.mpn_mpnet_train_get_state(h, 0, *tower0, s), ESTATE, "mpn_mpnet_train_get_state", "no mpn_mpnet_train_begin")
    _refused(lib, lib.mpn_mpnet_train_set_state(h, 0, *tower0, s), ESTATE, "mpn_mpnet_train_set_state", "no mpn_mpnet_train_begin")
    _refused(lib, lib.mpn_mpnet_train_get_head_state(h, *heads, C.byref(step), s), ESTATE, "mpn_mpnet_train_get_head_state", "no mpn_mpnet_train_begin")
    _refused(lib, lib.mpn_mpnet_train_set_head_state(h, *heads, 3, s), ESTATE, "mpn_mpnet_train_set_head_state", "no mpn_mpnet_train_begin")
    _refused(lib, lib.mpn_mpnet_train_scale_momentum(h, f(0.5), s), ESTATE, "mpn_mpnet_train_scale_momentum", "no mpn_mpnet_train_begin")
    _refused(lib, lib.mpn_frcnn_train_scale_momentum(plain._h, f(0.5), s), ESTATE, "mpn_frcnn_train_scale_momentum", "no mpn_frcnn_train_begin")
    assert step.value == -7
    for n_ in (net, twin):
        n_.tower_train_begin(momentum=0.9, weight_decay=5e-4)
        _tower_step(n_, dev, c, 0)
    plain.train_begin(depth=2)
    S0, P0 = _tower_state(net, dev), _plain_state_fc(plain, dev)
    # tower -1 and T
    for t in (-1, G.NT):
        _refused(lib, lib.mpn_mpnet_train_get_state(h, t, *tower0, s), EINVAL, "tower %d" % t, "T = 5")
        _refused(lib, lib.mpn_mpnet_train_set_state(h, t, *tower0, s), EINVAL, "tower %d" % t, "T = 5")
    # one NULL tensor in a set, a negative step
    for i, k in enumerate(("d_mix_v", "d_mix_vb", "d_fc6_v", "d_fc6_vb", "d_fc7_v", "d_fc7_vb")):
        args = list(tower0)
        args[i] = None
        _refused(lib, lib.mpn_mpnet_train_set_state(h, 1, *args, s), EINVAL, k + " is NULL")
    for i, k in enumerate(("d_cls_v", "d_cls_vb", "d_bbox_v", "d_bbox_vb")):
        args = list(heads)
        args[i] = None
        _refused(lib, lib.mpn_mpnet_train_set_head_state(h, *args, 3, s), EINVAL, k + " is NULL")
    _refused(lib, lib.mpn_mpnet_train_set_head_state(h, *heads, -1, s), EINVAL, "step -1 is negative")
    # factor NaN, inf, negative — both kinds
    for bad in (float("nan"), float("inf"), -0.5, -0.0):
        _refused(lib, lib.mpn_mpnet_train_scale_momentum(h, f(bad), s), EINVAL, "mpn_mpnet_train_scale_momentum", "factor")
        _refused(lib, lib.mpn_frcnn_train_scale_momentum(plain._h, f(bad), s), EINVAL, "mpn_frcnn_train_scale_momentum", "factor")
    # each kind refuses the other's handles, with the trainers' own message
    _refused(lib, lib.mpn_mpnet_train_get_state(plain._h, 0, *tower0, s), ESTATE, "not an mpn_mpnet_create handle")
    _refused(lib, lib.mpn_mpnet_train_set_state(plain._h, 0, *tower0, s), ESTATE, "not an mpn_mpnet_create handle")
    _refused(lib, lib.mpn_mpnet_train_get_head_state(plain._h, *heads, None, s), ESTATE, "not an mpn_mpnet_create handle")
    _refused(lib, lib.mpn_mpnet_train_set_head_state(plain._h, *heads, 0, s), ESTATE, "not an mpn_mpnet_create handle")
    _refused(lib, lib.mpn_mpnet_train_scale_momentum(plain._h, f(0.5), s), ESTATE, "not an mpn_mpnet_create handle")
    _refused(lib, lib.mpn_frcnn_train_scale_momentum(h, f(0.5), s), ESTATE, "cannot be trained")
    # rows pending: a set and a scale are refused, a get is not
    for j in range(2):
        G._add(net, dev, G._batch(3010 + j, 34 + 7 * j - 3, c["C"], 8))
    TR._add(plain, dev, TR._batch(3100, 30, PLAIN_C, 8))
    _refused(lib, lib.mpn_mpnet_train_set_state(h, 0, *tower0, s), ESTATE, "rows are pending")
    _refused(lib, lib.mpn_mpnet_train_set_head_state(h, *heads, 3, s), ESTATE, "rows are pending")
    _refused(lib, lib.mpn_mpnet_train_scale_momentum(h, f(0.5), s), ESTATE, "rows are pending")
    _refused(lib, lib.mpn_frcnn_train_scale_momentum(plain._h, f(0.5), s), ESTATE, "rows are pending")
    assert not _diff(_tower_state(net, dev), S0) and not _diff(_plain_state_fc(plain, dev), P0)   # nothing changed
    # ... and both handles train on: the pending rows' step equals the twin's, which saw no refused call
    net.tower_train_set_head(1 % c["K"])
    la, lb = net.tower_train_step(1e-3), _tower_step(twin, dev, c, 1)
    assert _bits(la.cpu().numpy(), lb.cpu().numpy())
    assert not G._all_bits(_tower_weights(net), _tower_weights(twin)) and not _diff(_tower_state(net, dev), _tower_state(twin, dev))
    assert np.isfinite(plain.train_step(1e-3).cpu().numpy()).all()
    plain.train_scale_momentum(0.5)
    net.tower_train_end()
    twin.tower_train_end()
    plain.train_end()


def _plain_state_fc(net, dev):
    """the plain handle's state at MPN_TRAIN_FC6 (no conv layer trained)"""
    S = net.train_state()
    torch.cuda.synchronize()
    out = {k: S[k].cpu().numpy() for k in PLAIN}
    out["step"] = S["step"]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. fit end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def _table_diff(pa, pb):
    from multipathnet_amd import t7
    A_, B_ = t7.load(pa), t7.load(pb)
    assert set(A_) == set(B_)
    return [k for k in A_ if (not _bits(A_[k], B_[k]) if isinstance(A_[k], np.ndarray) and A_[k].dtype == np.float32 else not np.array_equal(A_[k], B_[k]))]


def _fit_setup(kind, dev):
    """-> (make(weights or None) -> a net that has begun, add(net, case, draw, flip), weights(net), state(net), H, W, classes, K)"""
    from multipathnet_amd import train
    smp = train.DeviceRoiSampler(48, 0.25, 0.5, (0.1, 0.5), seed=321)
    if kind == "towers":
        def make(weights=None):
            net = G._net(G._params("A") if weights is None else weights, "A")
            net.tower_train_begin(momentum=0.9, weight_decay=5e-4, dropout=0.5, seed=SEED64)
            return net
        add = lambda net, case, draw, flip: net.tower_train_add_sampled(_t(case[0], dev), case[1], case[2], case[3], smp, draw, crowd_boxes=case[4], flip=flip)
        return make, add, _tower_weights, lambda net: _tower_state(net, dev), G.H, G.W, 5, 2

    def make(weights=None):
        P = dict(TR._params(PLAIN_FC, PLAIN_C))
        P.update(weights or {})
        net = TR._net(P)
        net.train_begin(depth=2, momentum=0.9, weight_decay=5e-4, dropout=0.5, seed=SEED64)
        return net
    add = lambda net, case, draw, flip: net.train_add_sampled(_t(case[0], dev), case[1], case[2], case[3], smp, draw, crowd_boxes=case[4], flip=flip)
    return make, add, _plain_weights, lambda net: _plain_state_fc(net, dev), TR.H, TR.W, PLAIN_C, 1


@pytest.mark.parametrize("kind", ["towers", "plain"])
def test_fit_equals_the_calls_by_hand_and_resumes_bit_for_bit(dev, tmp_path, kind):
    from multipathnet_amd import train
    make, add, weights, state, H_, W_, Cn, K = _fit_setup(kind, dev)
    cases = [GS._image_case(60 + i, H_, W_, Cn) for i in range(4)]
    EPOCHS, SIZE, LR = 4, 2, 1e-3

    def batch_fn_for(net):
        def batch_fn(e, it):   # a function of (epoch, it) alone: the draw counter is the sampler's whole state
            m = (e - 1) * SIZE + (it - 1)
            for j in range(2):
                n_bg, n_fg = add(net, cases[(m + j) % 4], 2 * m + j, bool(j))
                assert n_bg > 0 and n_fg > 0
            return m % K if K > 1 else None
        return batch_fn

    # by hand
    hand = make()
    fn, lr, losses = batch_fn_for(hand), LR, []
    for e in range(1, EPOCHS + 1):
        for it in range(1, SIZE + 1):
            k = fn(e, it)
            if kind == "towers":
                hand.tower_train_set_head(k)
            losses.append(hand.tower_train_step(lr) if kind == "towers" else hand.train_step(lr))
        if e % 2 == 0:
            lr = lr * 0.5
            (hand.tower_train_scale_momentum if kind == "towers" else hand.train_scale_momentum)(0.5)
    W_hand, S_hand = weights(hand), state(hand)
    losses = torch.stack(losses).cpu().numpy().astype(np.float64)

    # fit, with a validation that runs detect between the epochs
    rng = np.random.default_rng(8)
    vim, vbx = _t(rng.random((3, H_, W_), dtype=np.float32), dev), _t(G._boxes(rng, 40) * np.float32(min(H_ / G.H, W_ / G.W)), dev)
    net, logs, d1 = make(), [], tmp_path / "run"
    d1.mkdir()

    def validate(n, tag):
        scores, _ = n.detect(vim, vbx)
        return float(scores.sum())

    out = train.fit(net, batch_fn_for(net), EPOCHS, SIZE, LR, step=2, decay=0.5, snapshot=2, save_dir=str(d1), validate=validate, log=logs.append)
    assert out == LR * 0.5 * 0.5
    W_fit, S_fit = weights(net), state(net)
    assert not [n for n in W_fit if not _bits(W_fit[n], W_hand[n])] and not _diff(S_fit, S_hand) and S_fit["step"] == EPOCHS * SIZE
    assert any(not _bits(W_fit[n], weights(make())[n]) for n in ("cls_w", "bbox_w"))   # (it did train)
    assert sorted(os.listdir(str(d1))) == ["model_2.t7", "model_4.t7", "model_final.t7"]
    ep = [r for r in logs if "train_loss" in r]
    assert [r["learningRate"] for r in ep] == [LR, LR * 0.5, LR * 0.5, LR * 0.25] and len([r for r in logs if "validate" in r]) == 3
    for r in ep:   # the epoch's mean of the two losses (added in fp32 on the device: one rounding per step)
        m = losses[SIZE * (r["epoch"] - 1):SIZE * r["epoch"]].mean(0)
        assert abs(r["primary_loss"] - m[0]) <= 1e-6 * m[0] and abs(r["bboxregr_loss"] - m[1]) <= 1e-6 * m[1]

    # resumed from model_2.t7 on a rebuilt net
    ck = train.load_checkpoint(str(d1 / "model_2.t7"))
    assert ck["epoch"] == 2 and ck["learningRate"] == LR * 0.5 and ck["state"]["step"] == 2 * SIZE
    if kind == "towers":
        net.tower_train_end()
    else:
        net.train_end()
    net.close()
    del net
    again, d2 = make(ck["weights"]), tmp_path / "resumed"
    d2.mkdir()
    out2 = train.fit(again, batch_fn_for(again), EPOCHS, SIZE, 123.0, step=2, decay=0.5, snapshot=2, save_dir=str(d2), validate=validate, start=ck)
    assert out2 == out and sorted(os.listdir(str(d2))) == ["model_4.t7", "model_final.t7"]
    for f_ in ("model_4.t7", "model_final.t7"):
        assert not _table_diff(str(d1 / f_), str(d2 / f_)), f_
    W_res, S_res = weights(again), state(again)
    assert not [n for n in W_res if not _bits(W_res[n], W_hand[n])] and not _diff(S_res, S_hand)
