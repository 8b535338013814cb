"""Drawing a minibatch's rows on the device (mpn_attach_proposals, mpn_sample_rois, *_train_add_sampled)
against the numpy restatement of the two kernels (tests/sampler_np.py), bit for bit.

Every output buffer lies between guard zones — NaN for floats, a sentinel for integers — and is pre-filled with them, so a write outside
the rows a kernel owns, or a row it skips, shows.  Every case runs twice and the two runs must agree in every bit.
  attach      every (n, g, n_crowd) of sampler_np's lists; the inputs hold the edge cases tests/test_sampler_cpu.py proves on them
  sampler     records uploaded from the restatement (so attach is not judged twice): counts, background-first order, every drawn row,
              gt zeros and labels; exact thresholds; fewer rows than batch_size; flip; two draws; masked rows in neither set
  end to end  train_add_sampled + train_step against train_add of the restated rows + train_step: the same two losses and weights,
              on the tiny networks of the training tests (plain handle: depth 2 and one MPN_TRAIN_TRUNK depth; towers: network A)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_np as S  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = -7777777


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _p(t):
    return None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(dev, rows, cols, dtype):
    """(whole buffer, the view kernels write): GUARD elements before and behind, everything pre-filled with NaN / SENT"""
    n = rows * max(cols, 1)
    full = torch.full((n + 2 * GUARD,), float("nan") if dtype == torch.float32 else SENT, dtype=dtype, device=dev)
    view = full[GUARD:GUARD + n]
    return full, (view.view(rows, cols) if cols else view)


def _untouched(full, n_written):
    """the guard zones, and everything behind the first n_written elements of the view, still hold the fill"""
    h = full.cpu().numpy()
    rest = np.concatenate([h[:GUARD], h[GUARD + n_written:]])
    return bool(np.isnan(rest).all()) if h.dtype == np.float32 else bool((rest == SENT).all())


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and (a.view(np.uint8) == b.view(np.uint8)).all()


def _lib():
    import multipathnet_amd
    return multipathnet_amd.load()


def _check(rc, lib):
    assert rc == 0, lib.mpn_last_error()


# ---------------------------------------------------------------------------------------------------------------------------------
# attach
# ---------------------------------------------------------------------------------------------------------------------------------
def _attach_device(lib, dev, prop, gt, gl, crowds):
    m = len(prop) + len(gt)
    dp, dg, dl, dc = _t(prop, dev), _t(gt, dev), _t(gl, dev), _t(crowds, dev)
    bufs = [_guarded(dev, m, 4, torch.float32), _guarded(dev, m, 0, torch.float32), _guarded(dev, m, 0, torch.int32), _guarded(dev, m, 0, torch.int32)]
    _check(lib.mpn_attach_proposals(_p(dp), len(prop), _p(dg), _p(dl), len(gt), _p(dc), len(crowds), *[_p(v) for _, v in bufs], _stream()), lib)
    torch.cuda.synchronize()
    for (full, view) in bufs:
        assert _untouched(full, view.numel())
    return [v.cpu().numpy() for _, v in bufs]


@pytest.mark.parametrize("n", S.ATTACH_N)
def test_attach_equals_the_restatement(dev, n):
    lib = _lib()
    for (n_, g, c) in S.attach_cases():
        if n_ != n:
            continue
        prop, gt, gl, crowds = S.make_case(n, g, c)
        ref = S.attach(prop, gt, gl, crowds)
        runs = [_attach_device(lib, dev, prop, gt, gl, crowds) for _ in range(2)]
        for a, b in zip(*runs):
            assert _bits(a, b), ("two runs differ", n, g, c)
        boxes, overlap, corr, label = runs[0]
        assert not np.isnan(overlap).any() and not np.isnan(boxes).any(), (n, g, c)
        assert _bits(boxes, ref["boxes"]) and _bits(overlap, ref["overlap"]), (n, g, c)
        assert _bits(corr, ref["corr"]) and _bits(label, ref["label"]), (n, g, c)


def test_attach_python_wrapper(dev):
    from multipathnet_amd import train
    prop, gt, gl, crowds = S.make_case(65, 3, 2)
    rec, ref = train.attach_proposals_device(prop, gt, gl, crowd_boxes=crowds), S.attach(prop, gt, gl, crowds)
    assert _bits(rec["overlap"].cpu().numpy(), ref["overlap"]) and _bits(rec["correspondance"].cpu().numpy(), ref["corr"])
    assert _bits(rec["label"].cpu().numpy(), ref["label"]) and _bits(rec["boxes"].cpu().numpy(), ref["boxes"])
    host = train.attach_proposals(prop, gt, gl, crowd_boxes=crowds)
    assert _bits(rec["overlap"].cpu().numpy(), host["overlap"])
    smp = train.DeviceRoiSampler(16, 0.25, 0.5, (0.1, 0.5), seed=555)
    rois, gtb, labels = smp.sample(rec, draw=4)
    out = S.sample(ref, 16, 0.25, 0.5, 0.1, 0.5, 555, 4)
    assert smp.counts == out["counts"]
    assert _bits(rois.cpu().numpy(), out["rois"]) and _bits(gtb.cpu().numpy(), out["gt"]) and _bits(labels.cpu().numpy(), out["labels"])


# ---------------------------------------------------------------------------------------------------------------------------------
# sampler
# ---------------------------------------------------------------------------------------------------------------------------------
def _sample_device(lib, dev, rec, B, ff, ft, lo, hi, seed, draw, flip_width=0):
    from multipathnet_amd import _lib as L
    d = [_t(rec["boxes"], dev), _t(rec["overlap"], dev), _t(rec["corr"], dev), _t(rec["label"], dev)]
    m = rec["boxes"].shape[0]
    cfg = L.RoiSamplerCfg(B, ff, ft, lo, hi)
    bufs = [_guarded(dev, B, 4, torch.float32), _guarded(dev, B, 4, torch.float32), _guarded(dev, B, 0, torch.int32), _guarded(dev, 2, 0, torch.int32)]
    _check(lib.mpn_sample_rois(*[_p(v) for v in d], m, C.byref(cfg), seed, draw, flip_width, *[_p(v) for _, v in bufs], _stream()), lib)
    torch.cuda.synchronize()
    counts = tuple(int(v) for v in bufs[3][1].cpu().numpy())
    bg_num, fg_num = S.quotas(B, ff)
    r = min(bg_num, counts[0]) + min(fg_num, counts[1])
    assert _untouched(bufs[0][0], 4 * r) and _untouched(bufs[1][0], 4 * r) and _untouched(bufs[2][0], r) and _untouched(bufs[3][0], 2), "a write past row r"
    return {"rois": bufs[0][1][:r].cpu().numpy(), "gt": bufs[1][1][:r].cpu().numpy(), "labels": bufs[2][1][:r].cpu().numpy(), "counts": counts, "r": r}


def _same(out, ref):
    return (out["counts"] == ref["counts"] and _bits(out["rois"], ref["rois"]) and _bits(out["gt"], ref["gt"]) and _bits(out["labels"], ref["labels"]))


@pytest.mark.parametrize("name", list(S.SAMPLE_CASES))
def test_sampler_equals_the_restatement(dev, name):
    lib = _lib()
    n, g, c, B, ff, ft, lo, hi = S.SAMPLE_CASES[name]
    prop, gt, gl, crowds = S.make_case(n, g, c)
    rec = S.attach(prop, gt, gl, crowds)
    ref = S.sample(rec, B, ff, ft, lo, hi, 555, 1)
    assert ref["counts"][0] >= 1 and ref["counts"][1] >= 1, "a case may not pass by being empty"
    out, again = (_sample_device(lib, dev, rec, B, ff, ft, lo, hi, 555, 1) for _ in range(2))
    assert _same(out, again), "two runs differ"
    assert out["counts"] == ref["counts"], (out["counts"], ref["counts"])
    assert out["r"] == ref["r_bg"] + ref["r_fg"]
    assert _same(out, ref)
    r_bg = ref["r_bg"]
    assert (out["labels"][:r_bg] == 0).all() and (out["gt"][:r_bg] == 0).all() and (out["labels"][r_bg:] > 0).all(), "background first"
    if c:  # rows at -1 exist and are in neither set
        assert (rec["overlap"] == -1).any() and (rec["overlap"][ref["rows"]] != -1).all()
        assert ref["counts"][0] + ref["counts"][1] <= (rec["overlap"] != -1).sum()
    if name == "m60_few_fg":
        assert ref["r_fg"] == ref["counts"][1] < S.quotas(B, ff)[1] and out["r"] < B
    if name == "m68_many_fg":
        assert ref["counts"][1] > S.quotas(B, ff)[1] == ref["r_fg"]
    # another draw gives other rows, a 64-bit draw counter and seed are honoured, the same (seed, draw) the same rows
    for seed, draw in ((555, 2), (555, 1 + (1 << 32)), (555 + (1 << 40), 1)):
        other = _sample_device(lib, dev, rec, B, ff, ft, lo, hi, seed, draw)
        assert _same(other, S.sample(rec, B, ff, ft, lo, hi, seed, draw)), (seed, draw)
        assert not _bits(other["rois"], out["rois"]), (seed, draw)


@pytest.mark.parametrize("name", ["m60_few_fg", "m2114_crowds"])
def test_sampler_flip_equals_flip_boxes_of_the_unflipped_sample(dev, name):
    lib = _lib()
    n, g, c, B, ff, ft, lo, hi = S.SAMPLE_CASES[name]
    prop, gt, gl, crowds = S.make_case(n, g, c)
    rec = S.attach(prop, gt, gl, crowds)
    Wd = 1203
    plain = _sample_device(lib, dev, rec, B, ff, ft, lo, hi, 555, 3)
    flipped, again = (_sample_device(lib, dev, rec, B, ff, ft, lo, hi, 555, 3, flip_width=Wd) for _ in range(2))
    assert _same(flipped, again)
    assert _same(flipped, S.sample(rec, B, ff, ft, lo, hi, 555, 3, flip_width=Wd))
    for key in ("rois", "gt"):
        src, dst = _t(plain[key], dev), torch.empty((plain["r"], 4), dtype=torch.float32, device=dev)
        _check(lib.mpn_flip_boxes(_p(src), plain["r"], Wd, _p(dst), _stream()), lib)
        torch.cuda.synchronize()
        assert _bits(flipped[key], dst.cpu().numpy()), key
    assert _bits(flipped["labels"], plain["labels"])


def test_sampler_threshold_boundaries_are_exact(dev):
    lib = _lib()
    ex = S.exact_threshold_records()
    # [1,1,10,10] against GT [1,1,10,5]: exactly 0.5 -> foreground at fg_thr 0.5, not background at bg_hi 0.5
    rec = ex["half"]
    assert rec["overlap"][1] == np.float32(0.5)
    ref = S.sample(rec, 8, 0.5, 0.5, 0.1, 0.5, 555, 0)
    assert 1 in ref["fg"] and 1 not in ref["bg"] and ref["counts"][0] >= 1 and ref["counts"][1] >= 1
    out = _sample_device(lib, dev, rec, 8, 0.5, 0.5, 0.1, 0.5, 555, 0)
    assert _same(out, ref) and out["counts"] == (len(ref["bg"]), len(ref["fg"]))
    # one float below the threshold it is the other way round
    lower = S.sample(rec, 8, 0.5, np.nextafter(np.float32(0.5), np.float32(1)), 0.1, np.nextafter(np.float32(0.5), np.float32(1)), 555, 0)
    assert 1 in lower["bg"] and 1 not in lower["fg"]
    thr = float(np.nextafter(np.float32(0.5), np.float32(1)))
    assert _same(_sample_device(lib, dev, rec, 8, 0.5, thr, 0.1, thr, 555, 0), lower)
    # against GT [1,1,1,10]: fl(0.1) -> background at bg_lo = 0.1f
    rec = ex["tenth"]
    assert rec["overlap"][1] == np.float32(0.1)
    ref = S.sample(rec, 8, 0.5, 0.5, 0.1, 0.5, 555, 0)
    assert 1 in ref["bg"] and ref["counts"][0] >= 1 and ref["counts"][1] >= 1
    assert _same(_sample_device(lib, dev, rec, 8, 0.5, 0.5, 0.1, 0.5, 555, 0), ref)
    up = float(np.nextafter(np.float32(0.1), np.float32(1)))
    ref_up = S.sample(rec, 8, 0.5, 0.5, up, 0.5, 555, 0)
    assert 1 not in ref_up["bg"]
    assert _sample_device(lib, dev, rec, 8, 0.5, 0.5, up, 0.5, 555, 0)["counts"] == ref_up["counts"]


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def _image_case(seed, H, W, n_classes, n=60, fg_free=False):
    """one image with 3 GT boxes, n proposals (jittered and shifted copies, one identical to the crowd) and one crowd strip inside it;
    fg_free: no GT box and proposals only — every row is background, so the sample has no foreground"""
    rng = np.random.default_rng(seed)
    im = rng.random((3, H, W), dtype=np.float32)
    gt = np.zeros((3, 4), np.float32)
    for j in range(3):
        x1, y1 = rng.integers(8, W - 70), rng.integers(8, H - 50)
        gt[j] = [x1, y1, x1 + rng.integers(24, 56), y1 + rng.integers(20, 40)]
    gl = rng.integers(1, n_classes, 3).astype(np.int32)
    crowd = np.array([[W - 9, 0, W - 2, 2 * H]], np.float32)
    prop = np.zeros((n, 4), np.float32)
    prop[0] = [W - 9, 1, W - 2, H - 1]   # inside the crowd strip: masked
    for i in range(1, n):
        b = gt[i % 3]
        d = rng.uniform(-2, 2, 4) if i % 2 else 0.45 * (b[2] - b[0]) * np.array([1, 0, 1, 0]) + rng.uniform(-1, 1, 4)
        prop[i] = np.clip(b + d.astype(np.float32), 1, [W, H, W, H])
    if fg_free:
        return im, prop, gt[:0], gl[:0], crowd
    return im, prop, gt, gl, crowd


def _restated_rows(case, smp, draw, flip, W):
    im, prop, gt, gl, crowd = case
    rec = S.attach(prop, gt, gl, crowd)
    out = S.sample(rec, smp.batch_size, smp.fg_fraction, smp.fg_threshold, smp.bg_threshold[0], smp.bg_threshold[1], smp.seed, draw, flip_width=W if flip else 0)
    assert out["counts"][0] >= 1 and out["counts"][1] >= 1 and (rec["overlap"] == -1).any()
    return out


FR_CFG = [8, 16, "P", 16, "P", 32]
FR_H, FR_W, FR_MAXR = 96, 160, 200


def _frcnn(fc=96, n_classes=7, **kw):
    from multipathnet_amd import models
    P = models.synthetic_params(FR_CFG, pooled=7, fc_dim=fc, n_classes=n_classes, seed=557, head_scale="trained")
    return models.FastRCNN(P, cfg=FR_CFG, pooled=7, spatial_scale=0.25, max_h=FR_H, max_w=FR_W, max_rois=FR_MAXR, nms_thresh=0.3, **kw)


def _head_bits(net):
    torch.cuda.synchronize()
    W = {k: v.cpu().numpy() for k, v in net.head_weights().items()}
    for l, (w, b) in enumerate(zip(*[net.trunk_weights()[k] for k in ("conv_w", "conv_b")])):
        W["conv_w.%d" % l], W["conv_b.%d" % l] = w.cpu().numpy(), b.cpu().numpy()
    return W


@pytest.mark.parametrize("flip", [False, True], ids=["upright", "flip"])
@pytest.mark.parametrize("begin", [dict(depth=2), dict(trunk_layers=3)], ids=["fc6", "trunk3"])
def test_frcnn_train_add_sampled_equals_train_add_of_the_restated_rows(dev, begin, flip):
    from multipathnet_amd import nn, train
    smp = train.DeviceRoiSampler(48, 0.25, 0.5, (0.1, 0.5), seed=777)
    cases = [_image_case(11, FR_H, FR_W, 7), _image_case(12, FR_H, FR_W, 7)]
    a, b = _frcnn(), _frcnn()
    a.train_begin(dropout=0.5, seed=9, **begin)
    b.train_begin(dropout=0.5, seed=9, **begin)
    for i, case in enumerate(cases):
        im = _t(case[0], dev)
        counts = a.train_add_sampled(im, case[1], case[2], case[3], smp, draw=40 + i, crowd_boxes=case[4], flip=flip)
        ref = _restated_rows(case, smp, 40 + i, flip, FR_W)
        assert counts == ref["counts"]
        b.train_add(nn.hflip(im) if flip else im, _t(ref["rois"], dev), _t(ref["gt"], dev), _t(ref["labels"], dev))
    la, lb = a.train_step(0.01), b.train_step(0.01)
    torch.cuda.synchronize()
    assert _bits(la.cpu().numpy(), lb.cpu().numpy()), (la, lb)
    assert np.isfinite(la.cpu().numpy()).all()
    Wa, Wb = _head_bits(a), _head_bits(b)
    for k in Wa:
        assert _bits(Wa[k], Wb[k]), k
    a.train_end(); b.train_end()


def test_frcnn_empty_sample_adds_nothing_and_overflow_changes_nothing(dev):
    from multipathnet_amd import _lib as L, train
    net = _frcnn()
    net.train_begin(depth=2)
    smp = train.DeviceRoiSampler(48, 0.25, 0.5, (0.0, 0.5), seed=777)
    empty = _image_case(13, FR_H, FR_W, 7, fg_free=True)
    n_bg, n_fg = net.train_add_sampled(_t(empty[0], dev), empty[1], empty[2], empty[3], smp, draw=1, crowd_boxes=empty[4])
    ref = S.sample(S.attach(empty[1], empty[2], empty[3], empty[4]), 48, 0.25, 0.5, 0.0, 0.5, 777, 1)
    assert (n_bg, n_fg) == ref["counts"] and n_fg == 0 and n_bg >= 1
    with pytest.raises(L.MpnError, match="no pending rows"):
        net.train_step(0.01)
    # overflow: 190 pending rows, the sample's r rows do not fit max_rois = 200; the step afterwards is the 190 rows' step
    case = _image_case(14, FR_H, FR_W, 7)
    twin = _frcnn()
    twin.train_begin(depth=2)
    rng = np.random.default_rng(5)
    c = rng.uniform([24, 24], [FR_W - 24, FR_H - 24], (190, 2))
    wh = rng.uniform(12, 44, (190, 2))
    rois = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    labels = rng.integers(0, 7, 190).astype(np.int32)
    for nt in (net, twin):
        nt.train_add(_t(case[0], dev), _t(rois, dev), _t(rois + np.float32(0.5), dev), _t(labels, dev))
    r = len(S.sample(S.attach(case[1], case[2], case[3], case[4]), 48, 0.25, 0.5, 0.0, 0.5, 777, 2)["labels"])
    assert 190 + r > FR_MAXR
    with pytest.raises(L.MpnError, match="exceed the handle's max_rois"):
        net.train_add_sampled(_t(case[0], dev), case[1], case[2], case[3], smp, draw=2, crowd_boxes=case[4])
    la, lb = net.train_step(0.01), twin.train_step(0.01)
    torch.cuda.synchronize()
    assert _bits(la.cpu().numpy(), lb.cpu().numpy())
    Wa, Wb = _head_bits(net), _head_bits(twin)
    for k in Wa:
        assert _bits(Wa[k], Wb[k]), k


TW_CFG = [8, 16, "P", 16, 24, "P", 32, 32, "P", 64, "P", 64]
TW_H, TW_W = 150, 250


def _mpnet():
    from multipathnet_amd import models
    P = models.synthetic_mpnet_params(TW_CFG, pooled=7, fc_dim=128, n_classes=5, n_integral=2, seed=557)
    return models.MultiPathNet(P, cfg=TW_CFG, pooled=7, spatial_scale=1.0 / 16, max_h=TW_H, max_w=TW_W, max_rois=200, nms_thresh=0.3)


def _tower_bits(net):
    torch.cuda.synchronize()
    P = net.tower_weights()
    out = {"t%d.%s" % (t, k): v.cpu().numpy() for t, Wt in enumerate(P["towers"]) for k, v in Wt.items() if hasattr(v, "cpu")}
    out.update({k: P[k].cpu().numpy() for k in ("cls_w", "cls_b", "bbox_w", "bbox_b")})
    return out


@pytest.mark.parametrize("flip", [False, True], ids=["upright", "flip"])
def test_tower_train_add_sampled_equals_tower_train_add_of_the_restated_rows(dev, flip):
    from multipathnet_amd import _lib as L, nn, train
    smp = train.DeviceRoiSampler(48, 0.25, 0.5, (0.1, 0.5), seed=321)
    case = _image_case(21, TW_H, TW_W, 5)
    a, b = _mpnet(), _mpnet()
    a.tower_train_begin(dropout=0.5, seed=9)
    b.tower_train_begin(dropout=0.5, seed=9)
    im = _t(case[0], dev)
    if not flip:  # an image without foreground adds nothing
        empty = _image_case(22, TW_H, TW_W, 5, fg_free=True)
        lo = train.DeviceRoiSampler(48, 0.25, 0.5, (0.0, 0.5), seed=321)
        n_bg, n_fg = a.tower_train_add_sampled(_t(empty[0], dev), empty[1], empty[2], empty[3], lo, draw=0, crowd_boxes=empty[4])
        assert n_fg == 0 and n_bg >= 1
        with pytest.raises(L.MpnError, match="no pending rows"):
            a.tower_train_step(0.01)
    counts = a.tower_train_add_sampled(im, case[1], case[2], case[3], smp, draw=7, crowd_boxes=case[4], flip=flip)
    ref = _restated_rows(case, smp, 7, flip, TW_W)
    assert counts == ref["counts"]
    b.tower_train_add(nn.hflip(im) if flip else im, _t(ref["rois"], dev), _t(ref["gt"], dev), _t(ref["labels"], dev))
    la, lb = a.tower_train_step(0.01), b.tower_train_step(0.01)
    torch.cuda.synchronize()
    assert _bits(la.cpu().numpy(), lb.cpu().numpy()) and np.isfinite(la.cpu().numpy()).all()
    Wa, Wb = _tower_bits(a), _tower_bits(b)
    assert len(Wa) > 10
    for k in Wa:
        assert _bits(Wa[k], Wb[k]), k
    a.tower_train_end(); b.tower_train_end()
