"""Resumable tower training without a GPU: the header and the binding carry the six new entry points, each
answers a NULL handle; train.fit's call sequence — rates, the momentum scaling, snapshots, validation, the integral head, a resumed
run — against a recording stand-in for the net; the checkpoint table functions on CPU tensors, bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mpn_mpnet_train_get_state", "mpn_mpnet_train_set_state", "mpn_mpnet_train_get_head_state", "mpn_mpnet_train_set_head_state",
       "mpn_frcnn_train_scale_momentum", "mpn_mpnet_train_scale_momentum")
A = dict(cfg=[8, 16, "P", 16, 24, "P", 32, 32, "P", 64, "P", 64], fc=128, C=5, K=2)   # tests/test_gpu_train_towers.py's network A


def test_header_and_binding_carry_the_entry_points():
    src = open(os.path.join(ROOT, "include", "mpn.h")).read()
    assert re.search(r"#define\s+MPN_VERSION\s+600\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lua = open(os.path.join(ROOT, "multipathnet_amd", "lua", "mpn_cdef.lua")).read()
    import multipathnet_amd
    for flavour in (None, "debug"):
        lib = multipathnet_amd._lib.load(flavour)
        for n in NEW:
            assert re.search(r"\bint\s+%s\s*\(" % n, code), n
            assert re.search(r"\bint\s+%s\s*\(" % n, lua), n
            assert getattr(lib, n).argtypes is not None, n   # _lib.load declared the prototype


def test_null_handle_is_an_argument_error_without_a_gpu():
    import multipathnet_amd
    lib = multipathnet_amd.load()
    f, step = ctypes.c_float, ctypes.c_long(-7)
    calls = {"mpn_mpnet_train_get_state": (None, 0) + (None,) * 7, "mpn_mpnet_train_set_state": (None, 0) + (None,) * 7,
             "mpn_mpnet_train_get_head_state": (None,) * 5 + (ctypes.byref(step), None),
             "mpn_mpnet_train_set_head_state": (None,) * 5 + (ctypes.c_long(0), None),
             "mpn_frcnn_train_scale_momentum": (None, f(0.1), None), "mpn_mpnet_train_scale_momentum": (None, f(0.1), None)}
    assert sorted(calls) == sorted(NEW)
    for n, args in calls.items():
        assert getattr(lib, n)(*args) == -1, n
        assert b"invalid argument" in lib.mpn_last_error(), n
    assert step.value == -7
    assert lib.mpn_version() == 600


# ---------------------------------------------------------------------------------------------------------------------------------
# fit against a recording stand-in
# ---------------------------------------------------------------------------------------------------------------------------------
class _StandIn(object):
    """what train.fit, save_checkpoint and resume touch of a MultiPathNet (mpnet=True) or a plain FastRCNN, every call recorded"""

    def __init__(self, mpnet, calls):
        self.is_mpnet, self.calls, self._dropout, self.step, self.n_integral = mpnet, calls, (0.5, 0xFEDCBA9876543210), 0, 1
        self.v = torch.zeros(3)

    def _step(self, lr):
        self.calls.append(("step", lr))
        self.step += 1
        self.v = self.v * 0.5 + 1.0
        return torch.tensor([1.0 + self.step, 0.25], dtype=torch.float32)

    def _scale(self, f):
        self.calls.append(("scale", f))
        self.v = self.v * f

    def _set_head(self, k):
        self.calls.append(("set_head", k))

    def _set_dropout(self, rate, seed):
        self.calls.append(("set_dropout", rate, seed))

    def _load(self, state):
        self.calls.append(("load_state", int(state["step"])))
        self.step = int(state["step"])
        self.v = (state["towers"][0]["mix_w"] if self.is_mpnet else state["fc6_w"]).clone()

    tower_train_step = train_step = _step
    tower_train_scale_momentum = train_scale_momentum = _scale
    tower_train_set_head = train_set_head = _set_head
    tower_train_set_dropout = train_set_dropout = _set_dropout
    tower_train_load_state = train_load_state = _load

    # (tiny tensors: the tables' contents are judged below, here the files only have to exist and carry the run's keys)
    def tower_weights(self):
        self.calls.append(("save",))
        one = torch.ones(3)
        T = dict(region=0, use4=1, use3=0, total_feat=3, mix_w=torch.ones(1, 3), **{k: one for k in ("mix_b", "fc6_w", "fc6_b", "fc7_w", "fc7_b")})
        return dict(towers=[T], cls_w=one, cls_b=one, bbox_w=one, bbox_b=one, conv_w=[one], conv_b=[one], n_integral=1, n_classes=3)

    def tower_train_state(self):
        S = {"towers": [{k: self.v for k in ("mix_w", "mix_b", "fc6_w", "fc6_b", "fc7_w", "fc7_b")}], "step": self.step}
        S.update({k: self.v for k in ("cls_w", "cls_b", "bbox_w", "bbox_b")})
        return S

    def head_weights(self):
        self.calls.append(("save",))
        return {k: torch.ones(3) for k in ("fc6_w", "fc6_b", "fc7_w", "fc7_b", "cls_w", "cls_b", "bbox_w", "bbox_b")}

    def trunk_weights(self):
        return {"conv_w": [torch.ones(3)], "conv_b": [torch.ones(3)]}

    def train_state(self):
        S = {k: self.v for k in ("fc6_w", "fc6_b", "fc7_w", "fc7_b", "cls_w", "cls_b", "bbox_w", "bbox_b")}
        S.update(conv_w=[None], conv_b=[None], step=self.step)
        return S


def _run_fit(mpnet, save_dir, start=None, lr=0.0123):
    from multipathnet_amd import train
    calls, logs = [], []
    net = _StandIn(mpnet, calls)

    def batch_fn(e, it):
        calls.append(("batch", e, it))
        return (e + it) % 2 if it != 2 else None   # iteration 2 of every epoch gives no head

    def validate(n, tag):
        assert n is net
        calls.append(("validate", tag))
        return {"tag": tag}

    out = train.fit(net, batch_fn, n_epochs=5, epoch_size=3, lr=lr, step=2, decay=0.1, snapshot=2, save_dir=str(save_dir), validate=validate,
                    log=logs.append, start=start)
    return calls, logs, out, net


@pytest.mark.parametrize("mpnet", [True, False])
def test_fit_call_sequence(tmp_path, mpnet):
    from multipathnet_amd import train
    lr = 0.0123
    calls, logs, out, net = _run_fit(mpnet, tmp_path, lr=lr)
    rates = [lr, lr, lr * 0.1, lr * 0.1, lr * 0.1 * 0.1]   # Python doubles, the reference's Lua arithmetic
    assert [c[1] for c in calls if c[0] == "step"] == [rates[e] for e in range(5) for _ in range(3)]
    assert out == lr * 0.1 * 0.1   # (epoch 5 is no multiple of 2)
    # the whole sequence, written out
    want = []
    for e in range(1, 6):
        for it in range(1, 4):
            want.append(("batch", e, it))
            if it != 2:
                want.append(("set_head", (e + it) % 2))
            want.append(("step", rates[e - 1]))
        if e % 2 == 0:
            want += [("scale", 0.1), ("save",), ("validate", str(e))]   # the drop first, then that epoch's file, then the validation
    want += [("save",), ("validate", "final")]
    assert calls == want
    assert sorted(os.listdir(str(tmp_path))) == ["model_2.t7", "model_4.t7", "model_final.t7"]
    # the epoch records: the rate behind the drop, the epoch's mean losses; each validation's result
    ep = [r for r in logs if "train_loss" in r]
    assert [r["epoch"] for r in ep] == [1, 2, 3, 4, 5]
    assert [r["learningRate"] for r in ep] == [lr, lr * 0.1, lr * 0.1, lr * 0.1 * 0.1, lr * 0.1 * 0.1]
    for r in ep:
        steps = [3 * (r["epoch"] - 1) + i for i in (1, 2, 3)]
        assert r["primary_loss"] == pytest.approx(np.mean([1.0 + s for s in steps]), rel=1e-6) and r["bboxregr_loss"] == pytest.approx(0.25)
        assert r["train_loss"] == r["primary_loss"] + r["bboxregr_loss"]
        assert set(r) == {"epoch", "learningRate", "train_loss", "primary_loss", "bboxregr_loss"}
    assert [r["validate"] for r in logs if "validate" in r] == [{"tag": "2"}, {"tag": "4"}, {"tag": "final"}]
    # the files carry the epoch and the rate BEHIND the drop, and the 64-bit seed
    ck = train.load_checkpoint(str(tmp_path / "model_2.t7"))
    assert ck["epoch"] == 2 and ck["learningRate"] == lr * 0.1 and ck["seed"] == 0xFEDCBA9876543210 and ck["dropout"] == 0.5
    assert ck["state"]["step"] == 6 and ck.get("kind") == ("mpnet" if mpnet else None)
    ckf = train.load_checkpoint(str(tmp_path / "model_final.t7"))
    assert ckf["epoch"] == 5 and ckf["learningRate"] == out and ckf["state"]["step"] == 15

    # a run resumed from model_2.t7 replays exactly the tail of the sequence, and ends in the same state
    d2 = tmp_path / "resumed"
    d2.mkdir()
    calls2, logs2, out2, net2 = _run_fit(mpnet, d2, start=ck, lr=123.0)   # (the rate comes from the file)
    tail = want[want.index(("validate", "2")) + 1:]
    assert calls2 == [("set_dropout", 0.5, 0xFEDCBA9876543210), ("load_state", 6)] + tail
    assert out2 == out and net2.step == net.step == 15
    assert (net2.v.numpy().view(np.uint32) == net.v.numpy().view(np.uint32)).all()
    assert [r for r in logs2 if "train_loss" in r] == ep[2:]
    assert sorted(os.listdir(str(d2))) == ["model_4.t7", "model_final.t7"]
    assert open(str(d2 / "model_final.t7"), "rb").read() == open(str(tmp_path / "model_final.t7"), "rb").read()


# ---------------------------------------------------------------------------------------------------------------------------------
# the checkpoint tables
# ---------------------------------------------------------------------------------------------------------------------------------
def _bits(a, b):
    a, b = np.ascontiguousarray(np.asarray(a)), np.ascontiguousarray(np.asarray(b))
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def _momentum_like(t, rng):
    """random values of t's shape with -0.0, subnormals and the largest finite number among them"""
    a = rng.standard_normal(tuple(t.shape)).astype(np.float32).reshape(-1)
    special = np.array([-0.0, 1e-42, -3e-45, np.finfo(np.float32).max, np.finfo(np.float32).tiny], np.float32)
    a[:min(a.size, special.size)] = special[:a.size]
    return torch.from_numpy(a.reshape(tuple(t.shape)))


def test_mpnet_checkpoint_table_round_trip_is_exact():
    from multipathnet_amd import models, t7, train
    P = models.synthetic_mpnet_params(A["cfg"], pooled=7, fc_dim=A["fc"], n_classes=A["C"], n_integral=A["K"], seed=557)
    rng = np.random.default_rng(3)
    names = ("mix_w", "mix_b", "fc6_w", "fc6_b", "fc7_w", "fc7_b")
    heads = ("cls_w", "cls_b", "bbox_w", "bbox_b")
    S = {"towers": [{k: _momentum_like(T[k], rng) for k in names} for T in P["towers"]], "step": 123456789}
    S.update({k: _momentum_like(P[k], rng) for k in heads})
    seed, lr = 0xFEDCBA9876543210, 1e-3 * 0.1 * 0.1
    tab = train.mpnet_checkpoint_table(P, S, 0.5, seed, epoch=2800, learning_rate=lr)
    assert tab["kind"] == "mpnet" and tab["n_towers"] == 5 and tab["n_integral"] == 2 and tab["n_classes"] == 5 and tab["seed"] == str(seed)
    assert tab["n_conv"] == len(P["conv_w"]) == 8
    ck = train.checkpoint_read(t7.loads(t7.dumps(tab)))
    assert ck["kind"] == "mpnet" and ck["seed"] == seed and ck["dropout"] == 0.5 and ck["epoch"] == 2800 and ck["learningRate"] == lr
    Wc, Sc = ck["weights"], ck["state"]
    assert Sc["step"] == 123456789 and len(Wc["towers"]) == len(Sc["towers"]) == 5
    for t, T in enumerate(P["towers"]):
        for k in names:
            assert _bits(Wc["towers"][t][k], T[k]) and _bits(Sc["towers"][t][k], S["towers"][t][k]), (t, k)
        for k in ("region", "use4", "use3", "total_feat"):
            assert Wc["towers"][t][k] == T[k] and isinstance(Wc["towers"][t][k], int), (t, k)
    for k in heads:
        assert _bits(Wc[k], P[k]) and _bits(Sc[k], S[k]), k
    for l in range(8):
        assert _bits(Wc["conv_w"][l], P["conv_w"][l]) and _bits(Wc["conv_b"][l], P["conv_b"][l]), l
    for k in ("bbox_mean", "bbox_std"):
        assert (k in Wc) == (P.get(k) is not None)
        if k in Wc:
            assert Wc[k] == [float(x) for x in P[k]]   # the doubles creation takes, unchanged
    assert Wc["n_integral"] == 2 and Wc["n_classes"] == 5 and Wc["conv345_norm"] is True
    # a file without the optional keys returns none
    ck0 = train.checkpoint_read(t7.loads(t7.dumps(train.mpnet_checkpoint_table(P, S, 0.0, 1))))
    assert "epoch" not in ck0 and "learningRate" not in ck0


def test_a_table_without_kind_is_a_plain_checkpoint_with_todays_keys():
    from multipathnet_amd import t7, train
    rng = np.random.default_rng(4)
    r = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    keys = ("fc6_w", "fc6_b", "fc7_w", "fc7_b", "cls_w", "cls_b", "bbox_w", "bbox_b")
    shp = {"fc6_w": (6, 8), "fc6_b": (6,), "fc7_w": (6, 6), "fc7_b": (6,), "cls_w": (3, 6), "cls_b": (3,), "bbox_w": (12, 6), "bbox_b": (12,)}
    Wt = {k: r(*shp[k]) for k in keys}
    Wt.update(conv_w=[r(4, 3, 3, 3), r(2, 4, 3, 3)], conv_b=[r(4), r(2)])
    St = {k: (_momentum_like(Wt[k], rng) if not k.startswith("fc6") else None) for k in keys}   # depth MPN_TRAIN_FC7 + the last conv layer
    St.update(conv_w=[None, _momentum_like(Wt["conv_w"][1], rng)], conv_b=[None, _momentum_like(Wt["conv_b"][1], rng)], step=7)
    seed = 0x8000000000000001
    tab = train.plain_checkpoint_table(Wt, St, 0.5, seed)
    want = set(keys) | {"conv_w.0", "conv_b.0", "conv_w.1", "conv_b.1", "v.conv_w.1", "v.conv_b.1", "step", "n_conv", "dropout", "seed"}
    want |= {"v." + k for k in keys if not k.startswith("fc6")}
    assert set(tab) == want   # no "kind", no "n_integral", no "epoch": exactly what save_checkpoint has always written
    ck = train.checkpoint_read(t7.loads(t7.dumps(tab)))
    assert set(ck) == {"weights", "state", "dropout", "seed"} and ck["seed"] == seed and ck["dropout"] == 0.5 and ck["state"]["step"] == 7
    for k in keys:
        assert _bits(ck["weights"][k], Wt[k])
        assert ck["state"][k] is None if St[k] is None else _bits(ck["state"][k], St[k])
    assert ck["state"]["conv_w"][0] is None and _bits(ck["state"]["conv_w"][1], St["conv_w"][1]) and _bits(ck["state"]["conv_b"][1], St["conv_b"][1])
    assert _bits(ck["weights"]["conv_w"][0], Wt["conv_w"][0]) and "n_integral" not in ck["weights"]
    tabK = train.plain_checkpoint_table(Wt, St, 0.5, seed, n_integral=3, epoch=4, learning_rate=0.5)
    assert set(tabK) == want | {"n_integral", "epoch", "learningRate"}
    with pytest.raises(ValueError):
        train.checkpoint_read(dict(tab, kind="resnet"))
