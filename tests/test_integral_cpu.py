"""The integral loss on the plain Fast R-CNN handle, the parts that need no GPU: the float64 helper
(tests/integral_np.py) against PyTorch-CPU float64 autograd + torch.optim.SGD, the per-head sampler (donkey.lua:38-41) against
train_np.setup_one_np at its thresholds, models.integral_params' surgery (model_utils.lua:275-317) and the new entry points'
argument checks."""
import ctypes
import os

import numpy as np
import torch

import integral_np as I
import train_np as T
from test_train_cpu import _batch, _hand_made, _head


def _khead(rng, K, K6=40, F=24, C=5):
    P = _head(rng, K6, F, C)
    P["cls_w"], P["cls_b"] = rng.normal(0, 0.3, (K * C, F)), rng.normal(0, 0.5, K * C)   # K DIFFERENT classifiers: a wrong head would show
    return P


def test_float64_helper_equals_torch_float64_autograd_on_the_selected_head():
    rng = np.random.default_rng(4242)
    K6, F, C, B, K = 40, 24, 5, 19, 3
    P = _khead(rng, K, K6, F, C)
    mean, std = [0.01, -0.02, 0.03, 0.0], [0.1, 0.1, 0.2, 0.2]
    b = _batch(rng, B, K6, C, n_bg=6, n_far=4)
    for k in range(K):
        rows = I.head_rows(K, k, C)
        other = np.ones(K * C, bool)
        other[rows] = False
        loss, G, d = I.loss_and_grads(P, *b, mean, std, K, k, bbox_weight=1.3, depth=2)
        assert (np.abs(d) < 1).any() and (np.abs(d) >= 1).any() and (b[3] == 0).any()
        # exact zeros on the unselected classifiers, something on the selected one
        assert (G["cls_w"][other] == 0).all() and (G["cls_b"][other] == 0).all() and np.abs(G["cls_w"][rows]).max() > 0
        # one plain-SGD step at lr 1 without momentum or decay: w_old - w_new is autograd's gradient
        Pt, lt = I.torch_steps(P, [b], [k], 1.0, K, depth=2, momentum=0.0, weight_decay=0.0, bbox_weight=1.3, mean=mean, std=std, dtype=torch.float64)
        for n in T.TENSORS:
            gt_ = np.asarray(P[n], np.float64) - Pt[n]
            assert np.abs(G[n] - gt_).max() <= 1e-12 * max(np.abs(gt_).max(), 1e-300), (k, n)
        assert (Pt["cls_w"][other] == P["cls_w"][other]).all() and (Pt["cls_b"][other] == P["cls_b"][other]).all()
        assert np.abs(np.array(loss) - np.array(lt[0])).max() <= 1e-12 * np.abs(np.array(lt[0])).max()
        # the selected head's numbers are train_np's on the head [cls_k | bbox]
        Pk = dict(P)
        Pk["cls_w"], Pk["cls_b"] = P["cls_w"][rows], P["cls_b"][rows]
        l1, G1, _ = T.loss_and_grads(Pk, *b, mean, std, 1.3, 2)
        assert l1 == loss and (G1["cls_w"] == G["cls_w"][rows]).all() and (G1["fc6_w"] == G["fc6_w"]).all()


def test_unselected_heads_are_stepped_like_torch_sgd():
    """three steps, heads 0, 1, 2 in turn, momentum and weight decay on: Sgd64 == torch.optim.SGD in float64 at every depth, and an
    unselected classifier moves (decay, then momentum)"""
    rng = np.random.default_rng(77)
    K6, F, C, B, K = 40, 24, 5, 17, 3
    P = _khead(rng, K, K6, F, C)
    mean, std = [0.0, 0.0, 0.0, 0.0], [0.1, 0.1, 0.2, 0.2]
    batches = [_batch(rng, B, K6, C, n_bg=5, n_far=3) for _ in range(3)]
    for depth in (0, 1, 2):
        ref = I.Sgd64(P, K, depth=depth, momentum=0.9, weight_decay=5e-4, mean=mean, std=std)
        losses = [ref.step(*b, lr=0.05, k=k)[0] for k, b in enumerate(batches)]
        Pt, lt = I.torch_steps(P, batches, [0, 1, 2], 0.05, K, depth=depth, momentum=0.9, weight_decay=5e-4, mean=mean, std=std, dtype=torch.float64)
        for n in T.TENSORS:
            assert np.abs(ref.P[n] - Pt[n]).max() <= 1e-12 * np.abs(Pt[n]).max(), (depth, n)
        assert np.abs(np.array(losses) - np.array(lt)).max() <= 1e-12 * np.abs(np.array(lt)).max()
    # after ONE step on head 0 the other heads' weights carry the decay alone, their biases nothing
    one = I.Sgd64(P, K, depth=2, momentum=0.9, weight_decay=5e-4, mean=mean, std=std)
    one.step(*batches[0], lr=0.05, k=0)
    rest = slice(C, K * C)
    assert np.abs(one.P["cls_w"][rest] - P["cls_w"][rest] * (1 - 0.05 * 5e-4)).max() <= 1e-15
    assert (one.P["cls_b"][rest] == P["cls_b"][rest]).all() and (one.P["cls_w"][rest] != P["cls_w"][rest]).any()
    # K = 1 is train_np
    P1 = _head(rng, K6, F, C)
    a, b_ = I.Sgd64(P1, 1, mean=mean, std=std), T.Sgd64(P1, mean=mean, std=std)
    assert a.step(*batches[0], lr=0.05, k=0)[0] == b_.step(*batches[0], lr=0.05)[0]
    assert all((a.P[n] == b_.P[n]).all() for n in T.TENSORS)


def test_integral_sampler_thresholds_and_sets():
    from multipathnet_amd import train
    prop, gt, gl = _hand_made()
    rec = train.attach_proposals(prop, gt, gl)
    # more overlaps between the thresholds than the hand-made record has: the band edges, inclusive below and exclusive above
    ov = np.array([1.0, 0.75, np.nextafter(np.float32(0.75), np.float32(0)), 0.7, 0.66, 0.65, 0.6, 0.58, 0.55, 0.52, 0.5,
                   np.nextafter(np.float32(0.5), np.float32(0)), 0.3, 0.1, np.nextafter(np.float32(0.1), np.float32(0)), 0.0], np.float32)
    s = train.IntegralSampler(6, batch_size=128, fg_fraction=0.25, rng=np.random.default_rng(3))
    assert len(s.samplers) == 6 and np.abs(np.array(s.thresholds) - np.array([0.5, 0.55, 0.6, 0.65, 0.7, 0.75])).max() < 1e-12
    seen = set()
    for k, t in enumerate([0.5, 0.55, 0.6, 0.65, 0.7, 0.75]):
        rs = s.samplers[k]
        assert np.float32(rs.fg_threshold) == np.float32(t) and rs.bg_threshold[0] == 0.1 and np.float32(rs.bg_threshold[1]) == np.float32(t)
        for o in (ov, rec["overlap"]):
            bg, fg = rs.setup_one(dict(rec, overlap=o))
            bg_np, fg_np = T.setup_one_np(o, fg_threshold=t, bg_threshold=(0.1, t))
            assert list(bg) == bg_np and list(fg) == fg_np and not set(bg_np) & set(fg_np)
        seen.add((len(bg_np), len(fg_np)))
        # sample(rec, k) is head k's sampler: background rows first, labels 0 there, and every foreground row clears head k's threshold
        rois, gtb, labels = s.sample(rec, k)
        bg, fg = rs.setup_one(rec)
        n_b, n_f = T.select_counts_np(len(bg), len(fg))
        assert len(labels) == n_b + n_f and (labels[:n_b] == 0).all() and (labels[n_b:] > 0).all()
        for i in range(n_b, n_b + n_f):
            assert any((rois[i] == rec["boxes"][j]).all() for j in fg)
    assert len(seen) > 1   # the thresholds really cut the record differently
    other = train.IntegralSampler(3, bg_threshold_min=0.0, bg_threshold_max=0.3)
    assert np.abs(np.array(other.thresholds) - np.array([0.3, 0.35, 0.4])).max() < 1e-12 and other.samplers[2].bg_threshold[0] == 0.0


def test_integral_params_clones_the_classifier():
    from multipathnet_amd import models
    P = models.synthetic_params([8, "P", 16], pooled=3, fc_dim=16, n_classes=5, seed=3)
    P["cls_b"] = torch.arange(5, dtype=torch.float32)
    Q = models.integral_params(P, 4)
    assert Q["n_integral"] == 4 and "n_integral" not in P
    assert Q["cls_w"].shape == (20, 16) and Q["cls_b"].shape == (20,)
    for k in range(4):
        assert torch.equal(Q["cls_w"][5 * k:5 * k + 5], P["cls_w"]) and torch.equal(Q["cls_b"][5 * k:5 * k + 5], P["cls_b"])
    assert Q["cls_w"].data_ptr() != P["cls_w"].data_ptr()             # clones, not views: training one head must not move another
    assert Q["bbox_w"] is P["bbox_w"] and Q["fc6_w"] is P["fc6_w"]    # everything else is shared
    one = models.integral_params(P, 1)
    assert one["n_integral"] == 1 and torch.equal(one["cls_w"], P["cls_w"])


def test_create_integral_argument_errors_do_not_need_a_gpu():
    import multipathnet_amd
    from multipathnet_amd import _lib
    lib = multipathnet_amd.load()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpn.h")).read()
    assert "#define MPN_MAX_INTEGRAL 8" in hdr
    KMAX = 8
    h = ctypes.c_void_p()
    nul = [None] * 11
    assert lib.mpn_frcnn_create_integral(*nul, 1, ctypes.byref(h)) == -1 and b"invalid argument" in lib.mpn_last_error()
    assert lib.mpn_frcnn_create_integral(*nul, 0, ctypes.byref(h)) == -1 and lib.mpn_frcnn_create_integral(*nul, KMAX + 1, ctypes.byref(h)) == -1
    assert not h.value
    # a complete descriptor with K out of range: refused on K, by name, before any pointer is followed or the device is touched
    cout, pool = (ctypes.c_int * 2)(8, 16), (ctypes.c_int * 2)(1, 0)
    c = _lib.FrcnnConfig()
    c.n_conv, c.conv_cout, c.pool_after = 2, ctypes.cast(cout, ctypes.POINTER(ctypes.c_int)), ctypes.cast(pool, ctypes.POINTER(ctypes.c_int))
    c.pooled_h = c.pooled_w = 7
    c.spatial_scale, c.fc_dim, c.n_classes, c.max_h, c.max_w, c.max_rois, c.top_k = 0.5, 16, 5, 32, 32, 16, 10
    buf = (ctypes.c_float * 4)()
    fp = ctypes.cast(buf, ctypes.c_void_p)
    arr = (ctypes.c_void_p * 2)(fp, fp)
    for K in (0, -1, KMAX + 1):
        assert lib.mpn_frcnn_create_integral(ctypes.byref(c), arr, arr, fp, fp, fp, fp, fp, fp, fp, fp, K, ctypes.byref(h)) == -1
        assert b"MPN_MAX_INTEGRAL" in lib.mpn_last_error() and not h.value
    c.n_classes = 257   # K > 1 classifiers beyond the integral score kernel's limit
    assert lib.mpn_frcnn_create_integral(ctypes.byref(c), arr, arr, fp, fp, fp, fp, fp, fp, fp, fp, 2, ctypes.byref(h)) == -1
    assert b"256" in lib.mpn_last_error() and not h.value
    assert lib.mpn_frcnn_create_integral(ctypes.byref(c), arr, arr, fp, fp, fp, fp, fp, fp, fp, fp, 1, None) == -1   # no `out`
    assert lib.mpn_frcnn_train_set_head(None, 0) == -1 and b"invalid argument" in lib.mpn_last_error()
    assert lib.mpn_frcnn_n_integral(None) == 0
