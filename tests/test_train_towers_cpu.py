"""tests/train_towers_np.py (the float64 restatement the device's tower training is judged against) equals PyTorch float64 autograd +
torch.optim.SGD on the same graph; the header declares the tower-training entry points; they answer a null handle without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import train_towers_np as TT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mpn_mpnet_train_begin", "mpn_mpnet_train_add", "mpn_mpnet_train_step", "mpn_mpnet_train_end", "mpn_mpnet_train_set_dropout",
       "mpn_mpnet_train_set_head", "mpn_mpnet_get_tower_weights", "mpn_mpnet_get_head_weights")
KCAT, C5, PP, F, C = (4, 7, 7, 9, 9), 4, 4, 6, 3   # five towers, the last the het tower


def _random_params(rng, K):
    P = {}
    for t, kc in enumerate(KCAT):
        P["t%d.mix_w" % t], P["t%d.mix_b" % t] = rng.normal(0, 0.4, (C5, kc)), rng.normal(0, 0.1, C5)
        P["t%d.fc6_w" % t], P["t%d.fc6_b" % t] = rng.normal(0, 0.3, (F, C5 * PP)), rng.normal(0, 0.1, F)
        P["t%d.fc7_w" % t], P["t%d.fc7_b" % t] = rng.normal(0, 0.4, (F, F)), rng.normal(0, 0.1, F)
    P["cls_w"], P["cls_b"] = rng.normal(0, 0.3, (K * C, 4 * F)), rng.normal(0, 0.1, K * C)
    P["bbox_w"], P["bbox_b"] = rng.normal(0, 0.3, (4 * C, F)), rng.normal(0, 0.1, 4 * C)
    return P


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("rate", [0.0, 0.5])
def test_numpy_restatement_equals_torch_autograd(K, rate):
    rng = np.random.default_rng(5 + K)
    P = _random_params(rng, K)
    mean, std = [0.0, 0.0, 0.0, 0.0], [0.1, 0.1, 0.2, 0.2]
    ref = TT.Sgd64(P, K, momentum=0.9, weight_decay=5e-4, bbox_weight=1.5, mean=mean, std=std)
    batches, l64 = [], []
    for step in range(3):
        B = 6 - step
        _, rois, gt, labels = TT.make_batch(40 + step, B, C, 2, 96, 160)
        xs = [rng.normal(0, 1, (B, kc, PP)) for kc in KCAT]
        drop = TT.masks(555, step, len(KCAT), B, F, rate) if rate else None
        k = step % K
        loss, d, gz = ref.step(xs, rois, gt, labels, 1e-2, k=k, drop=drop)
        assert (np.abs(d) < 1).any() and (np.abs(d) >= 1).any()
        other = np.ones(K * C, bool)
        other[k * C:(k + 1) * C] = False
        assert (gz[:, other] == 0).all()   # the classifiers not selected: an exactly zero gradient
        l64.append(loss)
        batches.append((xs, rois, gt, labels, k, drop))
    Pt, lt = TT.torch_steps(P, batches, 1e-2, K, momentum=0.9, weight_decay=5e-4, bbox_weight=1.5, mean=mean, std=std, dtype=torch.float64)
    for n in TT.names(len(KCAT)):
        assert not np.array_equal(ref.P[n], np.asarray(P[n], np.float64)), n   # every tensor moved
        err = np.abs(ref.P[n] - Pt[n]).max() / np.abs(Pt[n]).max()
        assert err <= 1e-10, (n, err)
    assert np.abs(np.array(l64) - np.array(lt)).max() <= 1e-10 * np.abs(np.array(lt)).max()


def test_towers_never_share_a_mask():
    m = TT.masks(555, 3, 5, 16, 128, 0.5)
    flat = [a for pair in m for a in pair]
    for i in range(len(flat)):
        assert 0.3 < (flat[i] > 0).mean() < 0.7
        for j in range(i):
            assert not np.array_equal(flat[i], flat[j])


def test_header_declares_the_tower_training_entry_points():
    src = open(os.path.join(ROOT, "include", "mpn.h")).read()
    assert re.search(r"#define\s+MPN_VERSION\s+600\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, code), n


def test_null_handle_is_an_argument_error_without_a_gpu():
    import multipathnet_amd
    lib = multipathnet_amd.load()
    lib.mpn_last_error.restype = ctypes.c_char_p
    lib.mpn_mpnet_train_set_dropout.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_long]
    f = ctypes.c_float
    calls = {"mpn_mpnet_train_begin": (None, f(0.9), f(5e-4), f(1.0)), "mpn_mpnet_train_add": (None, None, 8, 8, None, None, None, 1, None),
             "mpn_mpnet_train_step": (None, f(0.1), None, None), "mpn_mpnet_train_end": (None,), "mpn_mpnet_train_set_dropout": (None, 0.5, 1),
             "mpn_mpnet_train_set_head": (None, 0), "mpn_mpnet_get_tower_weights": (None, 0, None, None, None, None, None, None, None),
             "mpn_mpnet_get_head_weights": (None, None, None, None, None, None)}
    assert sorted(calls) == sorted(NEW)
    for n, args in calls.items():
        assert getattr(lib, n)(*args) == -1, n
        assert b"invalid argument" in lib.mpn_last_error(), n
    assert lib.mpn_version() == 600


@pytest.mark.parametrize("name", ["A", "B"])
def test_gpu_test_batches_exercise_every_tensor_and_both_branches(name):
    """The seeds of tests/test_gpu_train_towers.py's gradient cases, checked here with the float64 restatement fed a random operand of
    the right shape (non-negative pooled values, each map's slab normalised per ROI, x 1000): every tensor's gradient has a non-zero
    rms, the batch holds both smooth-L1 branches, background and foreground rows."""
    import test_gpu_train_towers as G
    from multipathnet_amd import models
    c = G.CONFIGS[name]
    P0 = TT.flat(G._params(name))
    t3, t4 = models.conv_tap_indices(c["cfg"])
    cout, _ = models.cfg_layers(c["cfg"])
    widths = [[cout[-1]] + ([cout[t4]] if T["use4"] else []) + ([cout[t3]] if T["use3"] else []) for T in models.MPN_TOWERS]
    rng = np.random.default_rng(11)
    for case, spec in G.GRAD_BATCHES.items():
        if case == "B1":
            continue   # (one foreground row: the B > 1 conditions do not apply; the rms condition is asserted on the device's operand)
        parts = [G._batch(1000 + 17 * i + c["fc"], n, c["C"], n_bg) for i, (n, n_bg) in enumerate(spec)]
        rois, gt, labels = G._join(parts)
        B = len(labels)
        xs = []
        for ws in widths:
            slabs = [np.abs(rng.normal(0, 1, (B, w, G.PP))) for w in ws]
            xs.append(np.concatenate([1000.0 * s / np.sqrt((s * s).sum((1, 2), keepdims=True) + 1e-10) for s in slabs], 1))
        _, Gr, d, _ = TT.loss_and_grads(P0, xs, rois, gt, labels, c["K"], 0, G.MEAN, G.STD)
        assert (np.abs(d) < 1).any() and (np.abs(d) >= 1).any() and (labels == 0).any() and (labels > 0).any()
        for n_, g in Gr.items():
            assert np.sqrt((g * g).mean()) > 0, (case, n_)
