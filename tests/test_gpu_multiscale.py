"""Multi-scale testing (Fast R-CNN's image pyramid) on the device: mpn_project_im_rois_levels and the pyramid path of
mpn_frcnn_detect / mpn_frcnn_test_one (mpn_frcnn_set_scales) against tests/multiscale_np.py and the oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

import multiscale_np as M

pytestmark = pytest.mark.gpu

CFG = [8, 16, "P", 16, 24, "P", 32, 32, "P", 64, "P", 64]   # test_gpu_pipeline.SMALL's trunk
H0, W0, TARGETS, MAX = 240, 400, [180, 240, 300], 500        # levels 180x300, 240x400, 300x500: canvas 300x500
FC, NC, N, SPATIAL = 128, 7, 200, 1 / 16
FRCNN_TARGETS = [480, 576, 688, 864, 1200]                    # Fast R-CNN's multi-scale test set


def _np_params(P):
    return {k: ([t.numpy() for t in v] if isinstance(v, list) and v and hasattr(v[0], "numpy") else (v.numpy() if hasattr(v, "numpy") else v))
            for k, v in P.items()}


def _boxes(rng, n, W, H, lo=4, hi=None):
    hi = hi or min(W, H)
    c = rng.uniform([1, 1], [W, H], (n, 2))
    wh = np.exp(rng.uniform(np.log(lo), np.log(hi), (n, 2)))
    return np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 1, [W, H, W, H]).astype(np.float32)


def _oracle_maps(O, im, Pn, scales, cfg, trunk=None):
    """rules 1-2: each level resampled and transformed as the pipeline does (mpn_image_scale on the raw image, then the transformer),
    zero-padded top-left into the canvas, the whole trunk on the canvas; duplicate scales share the first level's map"""
    H, W = im.shape[1:]
    Hc, Wc = M.canvas(H, W, scales)
    maps = {}
    for l in M.distinct_levels(scales):
        h, w = M.level_size(H, W, scales[l])
        x = im if scales[l] == 1.0 else O.image_scale(im, h, w)
        x = O.image_transform(x, **O.ROSS)
        cv = np.zeros((3, Hc, Wc), np.float32)
        cv[:, :h, :w] = x
        maps[l] = trunk(cv) if trunk else O.vgg_trunk(cv, Pn["conv_w"], Pn["conv_b"], cfg)
    return np.stack([maps[scales.index(s)] for s in scales])


@pytest.fixture(scope="module")
def model(O, dev):
    from multipathnet_amd import models
    P = models.synthetic_params(CFG, pooled=7, fc_dim=FC, n_classes=NC, seed=557)
    Pn = _np_params(P)
    im = np.random.default_rng(901).random((3, H0, W0), dtype=np.float32)
    boxes = _boxes(np.random.default_rng(902), N, W0, H0)
    # large proposals for the coarse levels (area > 64225 -> s = 0.75, 39162 .. 64225 -> s = 1; everything smaller -> s = 1.25)
    boxes[:6] = [[1, 1, 400, 240], [1, 1, 300, 230], [50, 8, 340, 236], [10, 10, 230, 230], [5, 5, 215, 215], [100, 20, 330, 220]]
    scales = M.level_scales(H0, W0, TARGETS, MAX)
    maps = _oracle_maps(O, im, Pn, scales, CFG)
    rois, lv = M.project(boxes, scales)
    return dict(P=P, Pn=Pn, im=im, boxes=boxes, scales=scales, maps=maps, rois=rois, lv=lv)


def _net(model, **kw):
    from multipathnet_amd import models
    kw.setdefault("scale", TARGETS)
    kw.setdefault("max_size", MAX)
    kw.setdefault("max_h", 300)
    kw.setdefault("max_w", 500)
    return models.FastRCNN(model["P"], cfg=CFG, pooled=7, spatial_scale=SPATIAL, max_rois=N, **kw)


def _dev(model, dev):
    return torch.from_numpy(model["im"]).to(dev), torch.from_numpy(model["boxes"]).to(dev)


def _f(t):
    from multipathnet_amd import nn
    return nn._f(t)


def test_project_levels_kernel_is_the_restatement(dev):
    from multipathnet_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(77)
    scales = M.level_scales(600, 1000, FRCNN_TARGETS, 2000)
    assert len(set(scales)) == 5
    n = 6000
    c = rng.uniform(1, 1000, (n, 2))
    wh = np.exp(rng.uniform(np.log(2), np.log(1500), (n, 2)))
    b = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    b[:8] = [[1, 1, 224, 224], [1, 1, 112, 112], [5, 5, 5, 5], [np.nan, 1, 9, 9], [1, 1, np.inf, 9], [-np.inf, 1, np.inf, 9],
             [1, 5, np.inf, 4], [3, 3, 2, 2]]
    ref, lv = M.project(b, scales)
    assert sorted(set(lv.tolist())) == [0, 1, 2, 3, 4], "every distinct level must be chosen at least once"
    d_b = torch.from_numpy(b).to(dev)
    out = torch.full((n, 5), -7.0, dtype=torch.float32, device=dev)
    _lib.check(lib.mpn_project_im_rois_levels(_f(d_b), n, 5, (C.c_double * 5)(*scales), _f(out), None), "project levels")
    got = out.cpu().numpy()
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(got[~np.isnan(ref)].view(np.uint32), ref[~np.isnan(ref)].view(np.uint32))   # bit for bit
    assert fin.sum() > 0.99 * ref.size
    # one scale: bit for bit mpn_project_im_rois
    for s in (1.0, 0.8, 1.6):
        one = torch.empty_like(out)
        _lib.check(lib.mpn_project_im_rois_levels(_f(d_b), n, 1, (C.c_double * 1)(s), _f(out), None), "levels, one scale")
        _lib.check(lib.mpn_project_im_rois(_f(d_b), n, C.c_double(s), _f(one), None), "project")
        a, e = out.cpu().numpy(), one.cpu().numpy()
        assert np.array_equal(np.isnan(a), np.isnan(e)) and np.array_equal(a[~np.isnan(a)].view(np.uint32), e[~np.isnan(e)].view(np.uint32))


@pytest.mark.parametrize("rule", [0, 1])
def test_pyramid_detect_vs_oracle(O, dev, model, rule):
    """rules 1-5 end to end: per-level maps, the projected table (bit for bit), scores and decoded boxes against the oracle's head over
    the stacked [S,C,h,w] maps — under both ROI bin rules"""
    net = _net(model, roi_bin_rule=rule)
    im, bx = _dev(model, dev)
    scores, bbox = net.detect(im, bx)
    torch.cuda.synchronize()
    assert sorted(set(model["lv"].tolist())) == [0, 1, 2]
    maps = model["maps"]
    for l in range(len(TARGETS)):
        f = net.debug_tensor("conv5.%d" % l, maps[l].shape).cpu().numpy()
        assert (np.abs(f - maps[l]) <= 1e-4 * np.maximum(1, np.abs(maps[l]))).all(), l
    assert np.array_equal(net.debug_tensor("rois", (N, 5)).cpu().numpy(), model["rois"])
    with O.roi_bin_rule(rule):
        logits, deltas = O.frcnn_head(maps, model["rois"], model["Pn"], pooled=7, spatial_scale=SPATIAL)
    assert np.abs(scores.cpu().numpy() - O.softmax(logits)).max() < 1e-4
    ref_bbox = O.clamp_boxes(O.bbox_decode(model["boxes"], deltas), W0, H0)
    assert np.abs(bbox.cpu().numpy() - ref_bbox).max() < 1e-4 * max(W0, H0)
    # the pixel-major pooling (default) and the C8P form agree bit for bit
    from conftest import hooks
    with hooks(roi_pool_pm=0):
        n2 = _net(model, roi_bin_rule=rule)
        s2, b2 = n2.detect(im, bx)
        torch.cuda.synchronize()
        n2.close()
    assert torch.equal(s2, scores) and torch.equal(b2, bbox)


def test_single_entry_duplicates_and_restore_are_bit_identical(dev, model):
    im, bx = _dev(model, dev)
    ref = _net(model, scale=240)
    s1, b1 = ref.detect(im, bx)
    one = _net(model, scale=[240])                      # a one-entry table is the scalar
    assert one.scales == [240.0]
    s, b = one.detect(im, bx)
    assert torch.equal(s, s1) and torch.equal(b, b1)
    dup = _net(model, scale=[240, 240])                 # [t, t] == [t]: the second level is never picked
    s, b = dup.detect(im, bx)
    assert torch.equal(s, s1) and torch.equal(b, b1)
    assert np.array_equal(dup.debug_tensor("conv5.1", (-1,)).cpu().numpy(), dup.debug_tensor("conv5.0", (-1,)).cpu().numpy())
    pyr = _net(model)
    sp, bp = pyr.detect(im, bx)
    assert not torch.equal(sp, s1)
    pyr.set_scales([240])                               # -> single scale 240
    s, b = pyr.detect(im, bx)
    assert torch.equal(s, s1) and torch.equal(b, b1)
    pyr.set_scales([])                                  # -> the creation-time scalar (the table's first entry)
    first = _net(model, scale=TARGETS[0])
    s, b = pyr.detect(im, bx)
    s0, b0 = first.detect(im, bx)
    assert torch.equal(s, s0) and torch.equal(b, b0)
    pyr.set_scales(TARGETS)
    from multipathnet_amd import _lib
    with pytest.raises(_lib.MpnError, match="cached"):  # set_scales drops the cached maps
        pyr.detect(im, bx, recompute_features=False)
    s, b = pyr.detect(im, bx)
    assert torch.equal(s, sp) and torch.equal(b, bp)
    # ROI permutation permutes the outputs; a prefix of the proposals is the prefix of the outputs; cached maps == recomputed
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5)).to(dev)
    s, b = pyr.detect(im, bx[perm].contiguous())
    assert torch.equal(s, sp[perm]) and torch.equal(b, bp[perm])
    s, b = pyr.detect(im, bx[:61].contiguous(), recompute_features=False)
    assert torch.equal(s, sp[:61]) and torch.equal(b, bp[:61])


def test_graphs_and_split3(O, dev, model):
    im, bx = _dev(model, dev)
    off = _net(model)
    d_off, n_off = off.test_one_async(im, bx)
    torch.cuda.synchronize()
    ref = d_off[: int(n_off.item())].clone()
    on = _net(model)
    on.set_graphs(True)
    for _ in range(4):
        d, n = on.test_one_async(im, bx)
        torch.cuda.synchronize()
        assert int(n.item()) == ref.shape[0] and torch.equal(d[: ref.shape[0]], ref)
    caps, reps = on.graph_stats()
    assert caps >= 1 and reps >= 1, (caps, reps)
    on.set_scales(TARGETS)                              # drops the captured graphs: the next calls capture afresh and still agree
    for _ in range(3):
        d, n = on.test_one_async(im, bx)
        torch.cuda.synchronize()
        assert torch.equal(d[: ref.shape[0]], ref)
    # MPN_FC_SPLIT3 on the pyramid: the bars the split3 tests hold against the fp32 pipeline (logits within 1e-4 of the oracle)
    s3 = _net(model, fc_arith="split3")
    sc3, _ = s3.detect(im, bx)
    torch.cuda.synchronize()
    logits, deltas = O.frcnn_head(model["maps"], model["rois"], model["Pn"], pooled=7, spatial_scale=SPATIAL)
    assert np.abs(s3.debug_tensor("cls", logits.shape).cpu().numpy() - logits).max() < 1e-4
    assert np.abs(s3.debug_tensor("bbox_raw", deltas.shape).cpu().numpy() - deltas).max() < 1e-4
    assert np.abs(sc3.cpu().numpy() - O.softmax(logits)).max() < 1e-4


def test_test_one_kept_detections_are_the_oracles_on_own_outputs(O, dev, model):
    net = _net(model)
    im, bx = _dev(model, dev)
    dets, n = net.test_one_async(im, bx)
    torch.cuda.synchronize()
    dets = dets[: int(n.item())].cpu().numpy()
    keep, idx, nk = [t.cpu().numpy() for t in net.nms_results()]
    scores, bbox = [t.cpu().numpy() for t in net.detect(im, bx)]
    per = []
    for j in range(1, NC):
        sb, src = O.select_scored(scores, bbox, j, -1.5)
        ref, ridx = O.nms(sb, 0.3, return_index=True)
        assert nk[j - 1] == ref.shape[0] and np.array_equal(keep[j - 1, :nk[j - 1]], ref)
        assert np.array_equal(idx[j - 1, :nk[j - 1]], src[ridx])
        per.append(ref)
    kept, _ = O.keep_top_k(per, 100)
    exp = np.concatenate([np.concatenate([k, np.full((k.shape[0], 1), j + 1, np.float32)], 1) for j, k in enumerate(kept) if k.size])
    assert dets.shape == exp.shape and np.array_equal(dets, exp)


@pytest.mark.parametrize("rbox,voting", [(False, False), (False, True), (True, False)])
def test_iterative_localisation_relevels_refined_boxes(O, dev, model, rbox, voting):
    """num_iter = 2: the refined boxes of pass 1 are levelled by rule 3 and pooled from the cached maps (project_im_rois(new_boxes,
    im_scales)); each pass against the oracle on the device's own previous pass, the per-class NMS (+ voting) bit for bit"""
    im, bx = _dev(model, dev)
    net = _net(model, num_iter=2, use_rbox_scores=rbox, bbox_voting=voting, bbox_vote_thresh=0.5)
    net.test_one_async(im, bx)
    torch.cuda.synchronize()
    keep, _, nk = [t.cpu().numpy() for t in net.nms_results()]
    one = _net(model)
    s1, b1 = one.detect(im, bx)                                        # the first pass, clamped (Tester_FRCNN.lua:75-78)
    nb = O.select_boxes(s1.cpu().numpy(), b1.cpu().numpy())
    s2, b2 = one.detect(im, torch.from_numpy(nb).to(dev), recompute_features=False, clamp=False)
    torch.cuda.synchronize()
    r2, lv2 = M.project(nb, model["scales"])
    assert np.array_equal(one.debug_tensor("rois", (N, 5)).cpu().numpy(), r2)
    logits, deltas = O.frcnn_head(model["maps"], r2, model["Pn"], pooled=7, spatial_scale=SPATIAL)
    assert np.abs(s2.cpu().numpy() - O.softmax(logits)).max() < 1e-4
    assert np.abs(b2.cpu().numpy() - O.bbox_decode(nb, deltas)).max() < 1e-4 * max(W0, H0)
    sc = [s1.cpu().numpy(), s2.cpu().numpy()]
    bb = [b1.cpu().numpy(), b2.cpu().numpy()]
    if rbox:
        sc, bb = sc[1:], bb[:1]
    sc, bb = np.concatenate(sc), np.concatenate(bb)
    assert keep.shape[1] == sc.shape[0]
    for j in range(1, NC):
        sb, _ = O.select_scored(sc, bb, j, -1.5)
        ref = O.nms(sb, 0.3)
        if voting:
            ref = O.bbox_vote(ref, sb, 0.5)
        assert nk[j - 1] == ref.shape[0] and np.array_equal(keep[j - 1, :nk[j - 1]], ref), j


def test_refusals(dev, model):
    from multipathnet_amd import _lib, detect, models
    im, bx = _dev(model, dev)
    net = _net(model)
    with pytest.raises(_lib.MpnError, match="canvas"):           # the 300 x 500 canvas does not fit a 300 x 400 pipeline
        _net(model, max_w=400).detect(im, bx)
    for call in (lambda: net.test_one_pipelined(im, bx),
                 lambda: net.test_one_pipelined_host(torch.from_numpy(model["im"]).pin_memory(), torch.from_numpy(model["boxes"]).pin_memory()),
                 lambda: net.shard_head(im, bx, 0, 1)):
        with pytest.raises(_lib.MpnError, match="pyramid"):
            call()
    net.test_one_async(im, bx)                                    # the handle is still usable
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        detect.ImageDetect(net, scale=[TARGETS[0]], max_size=MAX)  # one entry of the pyramid alone
    with pytest.raises(ValueError):
        detect.ImageDetect(net, scale=TARGETS[:2], max_size=MAX)
    with pytest.raises(ValueError):
        detect.ImageDetect(net, scale=TARGETS, max_size=1000)
    d = detect.ImageDetect(net, scale=TARGETS, max_size=MAX)       # the model's own table passes through
    sd, _ = d.detect(im, bx)
    s, _ = net.detect(im, bx)
    assert torch.equal(sd, s)
    with pytest.raises(ValueError):
        detect.Tester_FRCNN(_net(model, scale=240), scale=TARGETS, max_size=MAX)
    # MultiPathNet and ResNet handles name their kind
    mp = models.synthetic_mpnet_params(CFG, pooled=7, fc_dim=128, n_classes=5, n_integral=2, seed=11)
    with pytest.raises(_lib.MpnError, match="MultiPathNet"):
        models.MultiPathNet(mp, cfg=CFG, pooled=7, spatial_scale=1 / 16, max_h=300, max_w=500, max_rois=32, scale=TARGETS, max_size=MAX)
    R = models.synthetic_resnet_params(depth=0, n_classes=5, base_width=8, blocks=[1, 1, 1, 1], block_type="bottleneck", seed=3)
    rn = models.ResNetFRCNN(R, max_h=300, max_w=500, max_rois=32, top_k=10)
    with pytest.raises(_lib.MpnError, match="ResNet"):
        rn.set_scales(TARGETS)
    rn.set_scales([240])                                          # a single scale is every handle's


def test_fullsize_vgg16_five_scales(O, dev):
    """VGG-16 at bench.synthetic_inputs() with Fast R-CNN's five targets: max 1000 (canvas 600 x 1000, levels 0.8 / 0.96 / 1 and two
    duplicates of 1) against PyTorch-CPU per level on a 100-ROI sample; max 2000 (canvas 1200 x 2000) runs on a 1200 x 2000 handle"""
    import bench
    from multipathnet_amd import models
    from oracle import torch_ref
    import torch.nn.functional as F
    P = models.synthetic_params(seed=557)
    Pn = _np_params(P)
    im, boxes = bench.synthetic_inputs()
    H, W = im.shape[1:]
    scales = M.level_scales(H, W, FRCNN_TARGETS, 1000)
    net = models.FastRCNN(P, max_h=H, max_w=W, max_rois=boxes.shape[0], scale=FRCNN_TARGETS, max_size=1000)
    d_im, d_bx = torch.from_numpy(im).to(dev), torch.from_numpy(boxes).to(dev)
    scores, bbox = net.detect(d_im, d_bx)
    torch.cuda.synchronize()
    assert torch.isfinite(scores).all() and torch.isfinite(bbox).all()
    rois, lv = M.project(boxes, scales)
    assert lv.max() <= max(M.distinct_levels(scales)) == 2 and sorted(set(lv.tolist())) == [0, 1, 2]
    assert np.array_equal(net.debug_tensor("rois", rois.shape).cpu().numpy(), rois)
    C_ = P["cls_w"].shape[0]
    cls = net.debug_tensor("cls", (boxes.shape[0], C_)).cpu().numpy()
    raw = net.debug_tensor("bbox_raw", (boxes.shape[0], 4 * C_)).cpu().numpy()
    with torch_ref.threads(16):
        maps = _oracle_maps(O, im, Pn, scales, None, trunk=lambda x: torch_ref.vgg_trunk(x, P, models.VGG16_CFG))
        idx = np.random.default_rng(8).choice(boxes.shape[0], 100, replace=False)
        pooled, _ = O.roi_pool(maps, rois[idx], 7, 7, 1 / 16)
        with torch.no_grad():
            f = torch.from_numpy(pooled.reshape(100, -1))
            f = F.relu(F.linear(f, P["fc6_w"], P["fc6_b"]))
            f = F.relu(F.linear(f, P["fc7_w"], P["fc7_b"]))
        logits, deltas = torch_ref.heads(f, Pn, C_)
    assert np.abs(cls[idx] - logits).max() < 1e-4
    assert np.abs(raw[idx] - deltas).max() < 1e-4
    net.close()
    big = models.FastRCNN(P, max_h=1200, max_w=2000, max_rois=boxes.shape[0], scale=FRCNN_TARGETS, max_size=2000)
    s2, b2 = big.detect(d_im, d_bx)
    torch.cuda.synchronize()
    assert torch.isfinite(s2).all() and torch.isfinite(b2).all()
    sc2 = M.level_scales(H, W, FRCNN_TARGETS, 2000)
    assert M.canvas(H, W, sc2) == (1200, 2000)
    r2, lv2 = M.project(boxes, sc2)
    assert np.array_equal(big.debug_tensor("rois", r2.shape).cpu().numpy(), r2)
    assert big.debug_tensor("conv5.4", (512, 75, 125)).abs().max().item() > 0
    big.close()
