"""Training the head, the parts that need no GPU: the float64 helper (tests/train_np.py) against PyTorch-CPU float64 autograd and
torch.optim.SGD, utils.convertTo against utils.convertFrom's formula, and the host-side ROI sampler (multipathnet_amd/train.py)
against BatchProviderROI's rules."""
import numpy as np
import torch

import train_np as T


def _head(rng, K6=40, F=24, C=5):
    P = {"fc6_w": rng.normal(0, (2.0 / K6) ** 0.5, (F, K6)), "fc6_b": rng.normal(0, 0.1, F),
         "fc7_w": rng.normal(0, (2.0 / F) ** 0.5, (F, F)), "fc7_b": rng.normal(0, 0.1, F),
         "cls_w": rng.normal(0, 0.3, (C, F)), "cls_b": rng.normal(0, 0.5, C),
         "bbox_w": rng.normal(0, 0.05, (4 * C, F)), "bbox_b": rng.normal(0, 0.1, 4 * C)}
    return P


def _batch(rng, B, K6, C, n_bg, n_far):
    """rows 0..n_bg-1 background; the last n_far foreground rows regress to a GT box far away (|d| >= 1), the others to a nearby one"""
    x = np.maximum(rng.normal(0, 1, (B, K6)), 0)
    c = rng.uniform(30, 120, (B, 2))
    wh = rng.uniform(20, 50, (B, 2))
    rois = np.concatenate([c - wh / 2, c + wh / 2], 1)
    gt = rois + rng.normal(0, 1.0, (B, 4))
    gt[B - n_far:] = rois[B - n_far:] * 0.5 + np.array([60.0, 60.0, 140.0, 150.0])
    labels = rng.integers(1, C, B)
    labels[:n_bg] = 0
    gt[:n_bg] = 0
    return x, rois, gt, labels


def test_float64_helper_equals_torch_float64_autograd_and_sgd():
    rng = np.random.default_rng(42)
    K6, F, C, B = 40, 24, 5, 19
    P = _head(rng, K6, F, C)
    mean, std = [0.01, -0.02, 0.03, 0.0], [0.1, 0.1, 0.2, 0.2]
    batches = [_batch(rng, B, K6, C, n_bg=6, n_far=4) for _ in range(3)]
    for depth in (0, 1, 2):
        ref = T.Sgd64(P, depth=depth, momentum=0.9, weight_decay=5e-4, bbox_weight=1.3, mean=mean, std=std)
        losses = []
        for i, b in enumerate(batches):
            loss, d = ref.step(*b, lr=0.05)
            losses.append(loss)
            if i == 0:  # both smooth-L1 branches and background rows are present
                assert (np.abs(d) < 1).any() and (np.abs(d) >= 1).any() and (b[3] == 0).any()
        Pt, lt = T.torch_steps(P, batches, 0.05, depth=depth, momentum=0.9, weight_decay=5e-4, bbox_weight=1.3, mean=mean, std=std, dtype=torch.float64)
        for k in T.TENSORS:
            err = np.abs(ref.P[k] - Pt[k]).max() / max(np.abs(Pt[k]).max(), 1e-300)
            assert err <= 1e-12, (depth, k, err)
            if k not in T.TRAINED[depth]:
                assert (ref.P[k] == np.asarray(P[k])).all()
        assert np.abs(np.array(losses) - np.array(lt)).max() <= 1e-12 * np.abs(np.array(lt)).max()


def test_biases_never_decay_and_all_background_has_no_box_loss():
    rng = np.random.default_rng(7)
    P = _head(rng)
    x, rois, gt, labels = _batch(rng, 11, 40, 5, n_bg=11, n_far=0)
    ref = T.Sgd64(P, depth=0, momentum=0.9, weight_decay=0.01, mean=None, std=None)
    loss, d = ref.step(x, rois, gt, labels, lr=0.1)
    assert loss[1] == 0.0 and d.size == 0
    assert (ref.P["bbox_b"] == P["bbox_b"]).all()
    assert np.abs(ref.P["bbox_w"] - (P["bbox_w"] - 0.1 * 0.01 * P["bbox_w"])).max() == 0.0


def test_convert_to_inverts_convert_from():
    from multipathnet_amd import utils
    rng = np.random.default_rng(3)
    c = rng.uniform(50, 200, (64, 2))
    wh = rng.uniform(10, 90, (64, 2))
    box = torch.from_numpy(np.concatenate([c - wh / 2, c + wh / 2], 1))
    y = torch.from_numpy(rng.normal(0, 0.3, (64, 4)))
    # utils.convertFrom's formula (utils.lua:212-248) in float64 on the host
    xc, yc, w, h = (box[:, 0] + box[:, 2]) * 0.5, (box[:, 1] + box[:, 3]) * 0.5, box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
    xtc, ytc, wt, ht = xc + y[:, 0] * w, yc + y[:, 1] * h, w * torch.exp(y[:, 2]), h * torch.exp(y[:, 3])
    decoded = torch.stack([xtc - wt / 2, ytc - ht / 2, xtc + wt / 2, ytc + ht / 2], 1)
    back = utils.convertTo(box, decoded)
    assert back.dtype == torch.float64 and (back - y).abs().max() < 1e-12
    assert (T.convert_to(box.numpy(), decoded.numpy()) - back.numpy()).__abs__().max() < 1e-14
    f = utils.convertTo(box.float(), decoded.float())
    assert f.dtype == torch.float32 and (f.double() - y).abs().max() < 1e-4


def _hand_made():
    # one GT box 100 x 100 (+1 convention: 101 x 101 pixels) and proposals whose IoU with it is exactly computable
    gt = np.array([[101.0, 101.0, 201.0, 201.0], [300.0, 50.0, 340.0, 130.0]], np.float32)
    gl = [3, 5]
    prop = np.array([
        [101, 101, 201, 201],      # IoU 1 with GT 0
        [101, 101, 201, 150],      # 101*50 / 101*101 = 0.495.. -> background
        [101, 101, 201, 151],      # 101*51 / 101*101 = 0.50495 -> foreground
        [101, 101, 201, 110],      # 10 / 101 = 0.099 -> below the background band
        [400, 300, 450, 350],      # IoU 0
        [300, 50, 340, 89],        # with GT 1: 40 / 81 = 0.4938 -> background
        [300, 50, 340, 130],       # IoU 1 with GT 1
    ], np.float32)
    return prop, gt, gl


def test_attach_proposals_and_sampler_rules():
    from multipathnet_amd import train
    prop, gt, gl = _hand_made()
    rec = train.attach_proposals(prop, gt, gl)
    n_gt = len(gt)
    assert rec["boxes"].shape == (n_gt + len(prop), 4) and (rec["boxes"][:n_gt] == gt).all() and (rec["boxes"][n_gt:] == prop).all()
    assert (rec["gt"] == np.array([1, 1] + [0] * len(prop), np.uint8)).all()
    # GT rows: overlap exactly 1 with themselves, foreground with their own class
    assert (rec["overlap"][:n_gt] == 1.0).all() and (rec["correspondance"][:n_gt] == [1, 2]).all() and (rec["label"][:n_gt] == gl).all()
    ov = rec["overlap"][n_gt:]
    want = np.array([1.0, 101 * 50 / (101 * 101), 101 * 51 / (101 * 101), 10 / 101, 0.0, 40 / 81, 1.0])
    assert np.abs(ov - want).max() < 1e-6
    assert (rec["correspondance"][n_gt:] == [1, 1, 1, 1, 0, 2, 2]).all()
    assert (rec["label"][n_gt:] == [3, 3, 3, 3, 0, 5, 5]).all()
    s = train.RoiSampler(batch_size=128, fg_fraction=0.25, rng=np.random.default_rng(0))
    bg, fg = s.setup_one(rec)
    bg_np, fg_np = T.setup_one_np(rec["overlap"])
    assert list(bg) == bg_np == [n_gt + 1, n_gt + 5] and list(fg) == fg_np == [0, 1, n_gt + 0, n_gt + 2, n_gt + 6]
    # thresholds: >= fg (inclusive), [lo, hi) for the background band
    edge = dict(rec, overlap=np.array([0.5, 0.1, np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.1), np.float32(0))], np.float32))
    bg_e, fg_e = s.setup_one(edge)
    assert list(fg_e) == [0] and list(bg_e) == [1, 2]
    assert T.setup_one_np(edge["overlap"]) == ([1, 2], [0])
    # counts are min(num, n) with replacement, background first, labels 0-based with 0 = background
    rois, gtb, labels = s.sample(rec)
    n_b, n_f = T.select_counts_np(len(bg), len(fg))
    assert (n_b, n_f) == (2, 5) and rois.shape == (7, 4) and gtb.shape == (7, 4) and labels.dtype == np.int32
    assert (labels[:n_b] == 0).all() and (labels[n_b:] > 0).all() and (gtb[:n_b] == 0).all()
    for i in range(n_b):
        assert any((rois[i] == rec["boxes"][j]).all() for j in bg)
    for i in range(n_b, n_b + n_f):
        j = [j for j in fg if (rois[i] == rec["boxes"][j]).all()]
        assert j and (gtb[i] == gt[rec["correspondance"][j[0]] - 1]).all() and labels[i] == rec["label"][j[0]]
    small = train.RoiSampler(batch_size=8, fg_fraction=0.25, rng=np.random.default_rng(1))
    rois, gtb, labels = small.sample(rec)
    assert T.select_counts_np(2, 5, 8, 0.25) == (2, 2) and len(labels) == 4 and (labels[:2] == 0).all() and (labels[2:] > 0).all()
    # no GT box at all: everything is overlap 0, nothing to sample
    none = train.attach_proposals(prop, np.zeros((0, 4), np.float32), [])
    assert (none["overlap"] == 0).all() and (none["label"] == 0).all() and len(s.sample(none)[2]) == 0


def test_bbox_regression_stats_follow_setup_data():
    from multipathnet_amd import train, utils
    prop, gt, gl = _hand_made()
    rec = train.attach_proposals(prop, gt, gl)
    mean, std = train.bbox_regression_stats([rec, rec])
    fg = np.nonzero(rec["overlap"] >= 0.5)[0]
    v = T.convert_to(rec["boxes"][fg], rec["boxes"][rec["correspondance"][fg] - 1])
    v = np.concatenate([v, v], 0)
    assert np.abs(mean - v.mean(0)).max() < 1e-6 and np.abs(std - v.std(0, ddof=1)).max() < 1e-6
    assert utils.convertTo(torch.from_numpy(gt), torch.from_numpy(gt)).abs().max() == 0
