"""Horizontal-flip test-time augmentation on the device (mpn_frcnn_set_augment, mpn_image_hflip, mpn_flip_boxes).
The standard throughout is bit equality with tests/augment_np.py's merge of two UNAUGMENTED detect calls on a plain handle built from
the same weights — (im, b) and (hflip(im), flipBoxes(b)): the trunk is deterministic, the rows are batch-invariant and the mirror is a
copy.  The one tolerance is the project's own against the oracle."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import augment_np as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = [8, 16, "P", 16, 24, "P", 32, 32, "P", 64, "P", 64]   # test_gpu_pipeline.SMALL's trunk
FC, NC, SPATIAL = 128, 7, 1 / 16


def _np_params(P):
    return {k: ([t.numpy() for t in v] if isinstance(v, list) and v and hasattr(v[0], "numpy") else (v.numpy() if hasattr(v, "numpy") else v))
            for k, v in P.items()}


def _boxes(rng, n, W, H, lo=8, hi=None):
    hi = hi or min(W, H)
    c = rng.uniform([1, 1], [W, H], (n, 2))
    wh = np.exp(rng.uniform(np.log(lo), np.log(hi), (n, 2)))
    return np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 1, [W, H, W, H]).astype(np.float32)


def _bits(a, b):
    """bit equality of two float32 arrays / tensors (NaNs must sit in the same places)"""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def _f(t):
    from multipathnet_amd import nn
    return nn._f(t)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _halves(plain, im, dev):
    """detect_half for augment_np: ImageDetect:detect (unclamped) of a PLAIN handle on the image or on its mirror"""
    imd, imf = _t(im, dev), _t(A.hflip(im), dev)

    def half(mirrored, boxes):
        s, b = plain.detect(imf if mirrored else imd, _t(boxes, dev), clamp=False)
        torch.cuda.synchronize()
        return s.cpu().numpy(), b.cpu().numpy()
    return half


def _check_detect(mk, im, boxes, dev):
    """the main check: detect(clamp = 0 / 1) of an augmented handle == augment_np.merge of two plain detect(clamp = 0) calls, bit for bit"""
    H, W = im.shape[1:]
    plain, aug = mk(augment=False), mk(augment=True)
    assert aug.augment and not plain.augment
    half = _halves(plain, im, dev)
    sA, bA = half(False, boxes)
    sB, bB = half(True, A.flip_boxes(boxes, W))
    assert np.isfinite(sA).all() and np.isfinite(bB).all()
    out = {}
    for clamp in (False, True):
        es, eb = A.merge(sA, bA, sB, bB, W, H, clamp=clamp)
        s, b = aug.detect(_t(im, dev), _t(boxes, dev), clamp=clamp)
        torch.cuda.synchronize()
        assert _bits(s, es), clamp
        assert _bits(b, eb), clamp
        out[clamp] = (s, b)
    assert not _bits(out[False][0], sA) and not _bits(out[False][1], bA)      # the second half really takes part
    s2, b2 = aug.detect(_t(im, dev), _t(boxes, dev), clamp=False)             # again on the same handle
    assert torch.equal(s2, out[False][0]) and torch.equal(b2, out[False][1])
    return plain, aug, out


@pytest.fixture(scope="module")
def vgg(dev):
    from multipathnet_amd import models
    P = models.synthetic_params(CFG, pooled=7, fc_dim=FC, n_classes=NC, seed=557)
    H, W, N = 150, 251, 200                                                   # an odd width: the mirror has no fixed column pair
    im = np.random.default_rng(1301).random((3, H, W), dtype=np.float32)
    boxes = _boxes(np.random.default_rng(1302), N, W, H)
    boxes[:4] = [[1, 1, W, H], [1, 1, 9, 9], [W - 8, H - 8, W, H], [100.5, 20.25, 180.75, 90.5]]
    return dict(P=P, Pn=_np_params(P), im=im, boxes=boxes, H=H, W=W, N=N)


def _vgg_net(vgg, **kw):
    from multipathnet_amd import models
    kw.setdefault("max_h", vgg["H"])
    kw.setdefault("max_w", vgg["W"])
    kw.setdefault("max_rois", vgg["N"])
    return models.FastRCNN(vgg["P"], cfg=CFG, pooled=7, spatial_scale=SPATIAL, **kw)


# ---- 1. the module entries -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(3, 5, 7), (1, 1, 1), (3, 4, 1), (3, 1, 2), (2, 37, 64), (3, 33, 255), (3, 600, 1000)])
def test_image_hflip_is_numpy_flip(dev, shape):
    from multipathnet_amd import _lib, nn
    lib = _lib.load()
    im = np.random.default_rng(shape[1] * 1000 + shape[2]).standard_normal(shape).astype(np.float32)
    im.flat[0] = np.nan
    d_in = _t(im, dev)
    out = torch.full(shape, -7.0, dtype=torch.float32, device=dev)
    _lib.check(lib.mpn_image_hflip(_f(d_in), shape[0], shape[1], shape[2], _f(out), None), "hflip")
    torch.cuda.synchronize()
    assert _bits(out, np.flip(im, 2))
    assert _bits(d_in, im)                                                    # the input is read only
    assert _bits(nn.hflip(d_in), A.hflip(im))
    assert lib.mpn_image_hflip(_f(d_in), shape[0], shape[1], shape[2], _f(d_in), None) == -1   # in place: refused, nothing written
    assert _bits(d_in, im)


@pytest.mark.parametrize("n,W", [(1, 1), (1, 7), (3, 251), (257, 250), (1000, 1000), (4096, 1 << 24)])
def test_flip_boxes_is_the_restatement(dev, n, W):
    from multipathnet_amd import _lib, utils
    lib = _lib.load()
    rng = np.random.default_rng(n + W)
    b = rng.uniform(-30, 1.1 * min(W, 5000) + 30, (n, 4)).astype(np.float32)
    b[0] = [1, 1, W, 9]
    if n > 2:
        b[1] = [np.nan, 2, np.inf, 3]
        b[2] = [16777215, 1, 0.5, 2]
    ref = A.flip_boxes(b, W)
    d_b = _t(b, dev)
    out = torch.full((n, 4), -7.0, dtype=torch.float32, device=dev)
    _lib.check(lib.mpn_flip_boxes(_f(d_b), n, W, _f(out), None), "flip_boxes")
    torch.cuda.synchronize()
    assert _bits(out, ref)
    assert _bits(utils.flipBoxes(d_b, W), ref)
    t5 = torch.cat([d_b, torch.arange(n, dtype=torch.float32, device=dev)[:, None]], 1)                 # a scored table keeps column 5
    assert _bits(utils.flipBoxes(t5, W), A.flip_boxes(t5.cpu().numpy(), W))
    _lib.check(lib.mpn_flip_boxes(_f(d_b), n, W, _f(d_b), None), "flip_boxes in place")                  # d_out may be d_boxes
    torch.cuda.synchronize()
    assert _bits(d_b, ref)


# ---- 2. the main check ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rule", [0, 1])
def test_vgg_detect_is_the_merge_of_two_plain_calls(dev, vgg, rule):
    plain, aug, out = _check_detect(lambda **kw: _vgg_net(vgg, roi_bin_rule=rule, **kw), vgg["im"], vgg["boxes"], dev)
    assert not _bits(out[True][1], out[False][1])                                                      # the clamp really clamps something
    # both maps stay cached: a detect on cached features gives the same rows, and a prefix of the boxes the prefix of the rows
    imd, bd = _t(vgg["im"], dev), _t(vgg["boxes"], dev)
    s, b = aug.detect(imd, bd, recompute_features=False, clamp=False)
    assert torch.equal(s, out[False][0]) and torch.equal(b, out[False][1])
    s, b = aug.detect(imd, bd[:1].contiguous(), recompute_features=False, clamp=True)                  # N = 1
    assert torch.equal(s, out[True][0][:1]) and torch.equal(b, out[True][1][:1])
    # ROI pooling straight from the C8P maps (debug flavour) agrees bit for bit
    from conftest import hooks
    with hooks(roi_pool_pm=0):
        n2 = _vgg_net(vgg, roi_bin_rule=rule, augment=True)
        s2, b2 = n2.detect(imd, bd, clamp=True)
        torch.cuda.synchronize()
        n2.close()
    assert _bits(s2, out[True][0]) and _bits(b2, out[True][1])


def test_vgg_detect_split3(dev, vgg):
    _check_detect(lambda **kw: _vgg_net(vgg, fc_arith="split3", **kw), vgg["im"], vgg["boxes"], dev)


@pytest.mark.parametrize("H0,W0", [(100, 151), (200, 320)])
def test_vgg_detect_where_getimages_rescales(dev, vgg, H0, W0):
    """scale_target set and s != 1 (1.5 up, 0.75 down): the ORIGINAL image is mirrored in front of getImages, the boxes are flipped with
    the ORIGINAL width, and the mirrored original may be larger than the pipeline's max_h x max_w"""
    from multipathnet_amd import _lib
    im = np.random.default_rng(H0).random((3, H0, W0), dtype=np.float32)
    boxes = _boxes(np.random.default_rng(W0), 120, W0, H0)
    assert _lib.load().mpn_pick_scale(H0, W0, 150.0, 400.0) != 1.0
    _check_detect(lambda **kw: _vgg_net(vgg, scale=150, max_size=400, max_h=150, max_w=240, **kw), im, boxes, dev)


def test_alexnet_detect(dev):
    from multipathnet_amd import models
    H, W, N = 160, 209, 40
    G = models.synthetic_alexnet_params(n_classes=6, seed=5, width=0.25, fc_dim=256)
    rng = np.random.default_rng(1311)
    _check_detect(lambda **kw: models.AlexNetFRCNN(G, max_h=H, max_w=W, max_rois=64, top_k=10, **kw),
                  rng.random((3, H, W), dtype=np.float32), _boxes(rng, N, W, H, lo=12), dev)


def test_multipathnet_detect(dev):
    from multipathnet_amd import models
    H, W, N = 150, 250, 117
    P = models.synthetic_mpnet_params(CFG, pooled=7, fc_dim=128, n_classes=9, n_integral=3, seed=11)
    rng = np.random.default_rng(1312)
    _check_detect(lambda **kw: models.MultiPathNet(P, cfg=CFG, pooled=7, spatial_scale=1 / 16, max_h=H, max_w=W, max_rois=N, **kw),
                  rng.random((3, H, W), dtype=np.float32), _boxes(rng, N, W, H, lo=12), dev)


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_resnet_detect(dev, bf16):
    from multipathnet_amd import models
    H, W, N = 120, 161, 50
    R = models.synthetic_resnet_params(depth=0, n_classes=5, base_width=8, blocks=[1, 1, 1, 2], block_type="bottleneck", seed=3)
    rng = np.random.default_rng(1313)
    _check_detect(lambda **kw: models.ResNetFRCNN(R, max_h=H, max_w=W, max_rois=64, top_k=10, bf16=bf16, **kw),
                  rng.random((3, H, W), dtype=np.float32), _boxes(rng, N, W, H, lo=12), dev)


def test_inception_detect(dev):
    from multipathnet_amd import models
    H, W, N = 150, 200, 48
    G = models.synthetic_inception_v3_params(n_classes=5, width=0.125, seed=9)
    rng = np.random.default_rng(1314)
    _check_detect(lambda **kw: models.InceptionFRCNN(G, max_h=H, max_w=W, max_rois=64, top_k=10, bf16=True, **kw),
                  rng.random((3, H, W), dtype=np.float32), _boxes(rng, N, W, H, lo=12), dev)


def test_vgg16_fullsize_detect_and_test_one(O, dev):
    """VGG-16 at bench.synthetic_inputs(): 600 x 1000 x 1000 ROIs (N == max_rois), detect bit for bit and the fused test_one's record"""
    import bench
    from multipathnet_amd import models
    P = models.synthetic_params(seed=557)
    im, boxes = bench.synthetic_inputs()
    H, W = im.shape[1:]
    N = boxes.shape[0]
    mk = lambda **kw: models.FastRCNN(P, max_h=H, max_w=W, max_rois=N, **kw)
    plain, aug, out = _check_detect(mk, im, boxes, dev)
    dets, n = aug.test_one_async(_t(im, dev), _t(boxes, dev))
    torch.cuda.synchronize()
    sc, bb = out[True][0].cpu().numpy(), out[True][1].cpu().numpy()
    per = [O.nms(O.select_scored(sc, bb, j, -1.5)[0], 0.3) for j in range(1, aug.n_classes)]
    kept, _ = O.keep_top_k(per, 100)
    exp = np.concatenate([np.concatenate([k, np.full((k.shape[0], 1), j + 1, np.float32)], 1) for j, k in enumerate(kept) if k.size])
    assert int(n.item()) == exp.shape[0] > 0 and np.array_equal(dets[: exp.shape[0]].cpu().numpy(), exp)
    plain.close()
    aug.close()
    torch.cuda.empty_cache()


# ---- 3. test_one ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("num_iter,rbox,voting,score_pow", [(1, False, False, 1.0), (1, False, True, 0.5), (2, False, False, 1.0), (2, True, False, 1.0),
                                                            (2, False, True, 1.0), (3, False, True, 0.5), (3, True, True, 1.0)])
def test_test_one_is_the_loop_around_two_plain_calls(O, dev, vgg, num_iter, rbox, voting, score_pow):
    """the boxes that reach the NMS == augment_np's loop (rule 6) around two plain detect calls per pass; from there the per-class keep
    lists, voting and top-k == the oracle's nms.c restatement on those tables, bit for bit; graphs on == graphs off; the host mirror
    (Tester_FRCNN with opt.test_augment) returns the same tables"""
    from multipathnet_amd import detect
    H, W, N = vgg["H"], vgg["W"], vgg["N"]
    kw = dict(num_iter=num_iter, use_rbox_scores=rbox, bbox_voting=voting, bbox_vote_thresh=0.5, bbox_vote_score_pow=score_pow)
    net = _vgg_net(vgg, augment=True, **kw)
    net.set_graphs(False)
    imd, bd = _t(vgg["im"], dev), _t(vgg["boxes"], dev)
    dets, n = net.test_one_async(imd, bd)
    torch.cuda.synchronize()
    dets = dets[: int(n.item())].cpu().numpy()
    keep, _, nk = [t.cpu().numpy() for t in net.nms_results()]
    plain = _vgg_net(vgg)
    sc, bb = A.tester_tables(_halves(plain, vgg["im"], dev), O.select_boxes, vgg["boxes"], W, H, num_iter=num_iter, use_rbox_scores=rbox)
    rows = (num_iter - 1 if rbox else num_iter) * N
    assert sc.shape[0] == rows == keep.shape[1]
    per = []
    for j in range(1, NC):
        sb, _ = O.select_scored(sc, bb, j, -1.5)
        ref = O.nms(sb, 0.3)
        if voting:
            votes = sb.copy()
            if score_pow != 1.0:
                votes[:, 4] = np.power(votes[:, 4].astype(np.float64), float(np.float32(score_pow))).astype(np.float32)
            ref = O.bbox_vote(ref, votes, 0.5)
        assert nk[j - 1] == ref.shape[0] and np.array_equal(keep[j - 1, : nk[j - 1]], ref, equal_nan=True), j
        per.append(ref)
    kept, _ = O.keep_top_k(per, 100)
    exp = np.concatenate([np.concatenate([k, np.full((k.shape[0], 1), j + 1, np.float32)], 1) for j, k in enumerate(kept) if k.size])
    assert dets.shape == exp.shape and dets.shape[0] > 0 and np.array_equal(dets, exp, equal_nan=True)
    # graphs on: captured once, replayed, the same record every time
    on = _vgg_net(vgg, augment=True, **kw)
    on.set_graphs(True)
    for _ in range(4):
        d, m = on.test_one_async(imd, bd)
        torch.cuda.synchronize()
        assert int(m.item()) == dets.shape[0] and np.array_equal(d[: dets.shape[0]].cpu().numpy(), dets, equal_nan=True)
    caps, reps = on.graph_stats()
    assert caps >= 1 and reps >= 1, (caps, reps)
    # the host mirror turns the option on in the module it is given and joins the same tables
    tester = detect.Tester_FRCNN(plain, opt={"test_augment": True, "test_num_iterative_loc": num_iter, "test_use_rbox_scores": rbox,
                                             "test_bbox_voting": voting, "test_bbox_voting_nms_threshold": 0.5,
                                             "test_bbox_voting_score_pow": score_pow})
    assert plain.augment
    img_boxes, (output, bbox_pred) = tester.testOne(imd, bd)
    assert _bits(output, sc) and _bits(bbox_pred, bb)
    for j, kb in enumerate(img_boxes):
        assert np.array_equal(keep[j, : nk[j]], kb.cpu().numpy(), equal_nan=True), j


# ---- 4. against the oracle -----------------------------------------------------------------------------------------------------

def test_small_vgg_vs_the_oracle_and_pytorch_cpu(O, dev, vgg):
    """the C oracle's and PyTorch-CPU's own unaugmented paths, called twice unchanged and merged by augment_np: scores within 1e-4,
    boxes within test_gpu_pipeline.py's decode tolerance (1e-4 of the image extent)"""
    from oracle import torch_ref
    H, W = vgg["H"], vgg["W"]
    im, boxes, Pn = vgg["im"], vgg["boxes"], vgg["Pn"]
    net = _vgg_net(vgg, augment=True)
    s, b = net.detect(_t(im, dev), _t(boxes, dev), clamp=False)
    sc, bc = net.detect(_t(im, dev), _t(boxes, dev), clamp=True)
    torch.cuda.synchronize()
    imf, bf = A.hflip(im), A.flip_boxes(boxes, W)
    sA, bA, _, _ = O.detect(im, boxes, Pn, cfg=CFG, target=H, max_size=W)
    sB, bB, _, _ = O.detect(imf, bf, Pn, cfg=CFG, target=H, max_size=W)
    for clamp, (ds, db) in ((False, (s, b)), (True, (sc, bc))):
        es, eb = A.merge(sA, bA, sB, bB, W, H, clamp=clamp)
        assert np.abs(ds.cpu().numpy() - es).max() < 1e-4
        assert np.abs(db.cpu().numpy() - eb).max() < 1e-4 * W

    def torch_half(image, bx):
        feat = torch_ref.vgg_trunk(O.image_transform(image, **O.ROSS), vgg["P"], CFG)
        logits, deltas = O.frcnn_head(feat, O.project_im_rois(bx, 1.0), Pn, pooled=7, spatial_scale=SPATIAL)
        return O.softmax(logits), O.bbox_decode(bx, deltas)
    with torch_ref.threads(16):
        tA, tB = torch_half(im, boxes), torch_half(imf, bf)
    es, eb = A.merge(tA[0], tA[1], tB[0], tB[1], W)
    assert np.abs(s.cpu().numpy() - es).max() < 1e-4
    assert np.abs(b.cpu().numpy() - eb).max() < 1e-4 * W


# ---- 5. off is off -------------------------------------------------------------------------------------------------------------

def test_off_is_byte_identical(dev, vgg):
    from multipathnet_amd import _lib
    imd, bd = _t(vgg["im"], dev), _t(vgg["boxes"], dev)
    kw = dict(num_iter=2, bbox_voting=True)

    def record(net):
        s, b = net.detect(imd, bd)
        s2, b2 = net.detect(imd, bd[:50].contiguous(), recompute_features=False, clamp=False)
        d, n = net.test_one_async(imd, bd)
        torch.cuda.synchronize()
        keep, idx, nk = net.nms_results()
        # the rows of a class's table behind its n_keep are not output: whatever an earlier image left there (the tables of an
        # augmented run keep more or fewer rows) — compare the kept rows only
        live = torch.arange(keep.size(1), device=keep.device)[None, :] < nk[:, None]
        keep = torch.where(live[:, :, None], keep, torch.zeros_like(keep))
        idx = torch.where(live, idx, torch.zeros_like(idx))
        return [t.clone() for t in (s, b, s2, b2, d[: int(n.item())], n, keep, idx, nk)]
    fresh = record(_vgg_net(vgg, **kw))                          # never called the setter
    net = _vgg_net(vgg, **kw)
    net.set_augment(True)
    on = record(net)
    assert not torch.equal(on[0], fresh[0])
    net.set_augment(False)
    assert not net.augment
    with pytest.raises(_lib.MpnError, match="cached"):            # the setter drops the cached maps
        net.detect(imd, bd, recompute_features=False)
    off = record(net)
    only_off = _vgg_net(vgg, **kw)
    only_off.set_augment(False)
    for got in (off, record(only_off), record(_vgg_net(vgg, augment=False, **kw))):
        assert len(got) == len(fresh)
        for x, y in zip(got, fresh):
            assert x.dtype == y.dtype and torch.equal(x, y)
    net.set_augment(True)                                         # and on again gives the augmented record again
    for x, y in zip(record(net), on):
        assert torch.equal(x, y)
    # with graphs: the setter drops the captured ones, the next calls capture afresh
    g = _vgg_net(vgg, **kw)
    g.set_graphs(True)
    for want, flag in ((fresh, False), (on, True), (fresh, False)):
        g.set_augment(flag)
        for _ in range(3):
            d, n = g.test_one_async(imd, bd)
            torch.cuda.synchronize()
            assert torch.equal(d[: int(n.item())], want[4])


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------

def _refused(call, word):
    from multipathnet_amd import _lib
    with pytest.raises(_lib.MpnError) as e:
        call()
    msg = str(e.value)
    assert "(status -1)" in msg, msg                               # MPN_EINVAL
    assert word in msg and len(msg.split("): ", 1)[1]) > 10, msg   # mpn_last_error() names the reason


def test_refusals_leave_the_handle_usable(dev, vgg):
    from multipathnet_amd import models
    imd, bd = _t(vgg["im"], dev), _t(vgg["boxes"], dev)
    net = _vgg_net(vgg, augment=True)
    d0, n0 = net.test_one_async(imd, bd)
    torch.cuda.synchronize()
    want = d0[: int(n0.item())].clone()
    for call in (lambda: net.test_one_pipelined(imd, bd),
                 lambda: net.test_one_pipelined_host(torch.from_numpy(vgg["im"]).pin_memory(), torch.from_numpy(vgg["boxes"]).pin_memory()),
                 lambda: net.shard_head(imd, bd, 0, 1)):
        _refused(call, "augmentation")
        d, n = net.test_one_async(imd, bd)
        torch.cuda.synchronize()
        assert torch.equal(d[: int(n.item())], want)
    # a pyramid and augmentation: whichever setter comes second refuses and changes nothing
    _refused(lambda: net.set_scales([120, 150, 180]), "augmentation")
    assert net.augment
    d, n = net.test_one_async(imd, bd)
    torch.cuda.synchronize()
    assert torch.equal(d[: int(n.item())], want)
    pyr = _vgg_net(vgg, scale=[120, 150, 180], max_size=300, max_h=180, max_w=302)
    sp, bp = pyr.detect(imd, bd)
    _refused(lambda: pyr.set_augment(True), "pyramid")
    assert not pyr.augment
    s, b = pyr.detect(imd, bd)
    assert torch.equal(s, sp) and torch.equal(b, bp)
    with pytest.raises(Exception):
        _vgg_net(vgg, scale=[120, 150, 180], max_size=300, max_h=180, max_w=302, augment=True)
    # the handle kinds that keep one trunk map: no iterative localisation under augmentation, no cached-features detect
    mp = models.synthetic_mpnet_params(CFG, pooled=7, fc_dim=128, n_classes=5, n_integral=2, seed=11)
    R = models.synthetic_resnet_params(depth=0, n_classes=5, base_width=8, blocks=[1, 1, 1, 1], block_type="bottleneck", seed=3)
    G = models.synthetic_alexnet_params(n_classes=6, seed=5, width=0.25, fc_dim=256)
    H, W = 150, 250
    rng = np.random.default_rng(1321)
    im2, bx2 = _t(rng.random((3, H, W), dtype=np.float32), dev), _t(_boxes(rng, 32, W, H, lo=12), dev)
    kinds = [("MultiPathNet", lambda **kw: models.MultiPathNet(mp, cfg=CFG, pooled=7, spatial_scale=1 / 16, max_h=H, max_w=W, max_rois=32, **kw)),
             ("ResNet", lambda **kw: models.ResNetFRCNN(R, max_h=H, max_w=W, max_rois=32, top_k=10, **kw)),
             ("op-list", lambda **kw: models.AlexNetFRCNN(G, max_h=H, max_w=W, max_rois=32, top_k=10, **kw))]
    for word, mk in kinds:
        it2 = mk(num_iter=2)
        d, n = it2.test_one_async(im2, bx2)
        torch.cuda.synchronize()
        ref = d[: int(n.item())].clone()
        _refused(lambda: it2.set_augment(True), word)
        assert not it2.augment
        d, n = it2.test_one_async(im2, bx2)
        torch.cuda.synchronize()
        assert torch.equal(d[: int(n.item())], ref)
        it2.set_augment(False)                                      # off is always accepted
        it2.close()
        one = mk(augment=True)
        s, b = one.detect(im2, bx2)
        _refused(lambda: one.detect(im2, bx2, recompute_features=False), word)
        s2, b2 = one.detect(im2, bx2)
        assert torch.equal(s, s2) and torch.equal(b, b2)
        one.set_augment(False)                                      # ... and drops the (mirrored) map the handle holds
        with pytest.raises(Exception, match="cached"):
            one.detect(im2, bx2, recompute_features=False)
        one.close()


# ---- 7. re-use -----------------------------------------------------------------------------------------------------------------

def test_fullsize_mixed_size_stream_on_one_augmented_handle(dev):
    """bench.MIXED_SIZES back to back on ONE augmented VGG-16 handle (s = 1, 1.25 up, the capped scale, 0.5 down — the 1200 x 1600
    original is larger than the pipeline's 1000 x 1000, so the mirror buffer grows; halos re-laid at every size change; ragged
    proposal counts) == a fresh augmented handle per image, records and raw tables"""
    import bench
    from multipathnet_amd import models
    P = models.synthetic_params(seed=557)
    stream = bench.mixed_size_inputs()
    mk = lambda: models.FastRCNN(P, max_h=1000, max_w=1000, max_rois=bench.N_ROIS, scale=600, max_size=1000, augment=True)
    ref = []
    for im, bx in stream:
        f = mk()
        imd, bd = _t(im, dev), _t(bx, dev)
        d, n = f.test_one_async(imd, bd)
        torch.cuda.synchronize()
        s, b = f.detect(imd, bd, clamp=False)
        ref.append((d[: int(n.item())].clone(), s.clone(), b.clone()))
        assert ref[-1][0].shape[0] > 0
        f.close()
        del f
        torch.cuda.empty_cache()
    net = mk()
    for i in (5, 0, 4, 3, 2, 1, 0, 0, 5, 3):
        im, bx = stream[i]
        imd, bd = _t(im, dev), _t(bx, dev)
        d, n = net.test_one_async(imd, bd)
        torch.cuda.synchronize()
        assert torch.equal(d[: int(n.item())], ref[i][0]), i
        s, b = net.detect(imd, bd, recompute_features=False, clamp=False)     # both cached maps are this image's
        assert torch.equal(s, ref[i][1]) and torch.equal(b, ref[i][2]), i
    net.close()
    torch.cuda.empty_cache()


# ---- the C host ----------------------------------------------------------------------------------------------------------------

def test_c_host_augment_flag_matches_the_python_host(dev, tmp_path):
    from multipathnet_amd import models
    H, W, N, Cn, fc = 150, 250, 120, 9, 128
    P = models.synthetic_params(CFG, pooled=7, fc_dim=fc, n_classes=Cn, seed=77)
    rng = np.random.default_rng(78)
    im = rng.random((3, H, W), dtype=np.float32)
    boxes = _boxes(rng, N, W, H, lo=12)
    couts = [c for c in CFG if c != "P"]
    pool_after = [1 if (i + 1 < len(CFG) and CFG[i + 1] == "P") else 0 for i, c in enumerate(CFG) if c != "P"]
    blob = [struct.pack("<%di" % (2 + 2 * len(couts) + 6), 0x4d504e31, len(couts), *couts, *pool_after, fc, Cn, 7, H, W, N)]
    f32 = lambda t: np.ascontiguousarray(t.numpy() if hasattr(t, "numpy") else t, dtype=np.float32).tobytes()
    for w, b in zip(P["conv_w"], P["conv_b"]):
        blob += [f32(w), f32(b)]
    for k in ("fc6_w", "fc6_b", "fc7_w", "fc7_b", "cls_w", "cls_b", "bbox_w", "bbox_b"):
        blob.append(f32(P[k]))
    blob += [f32(np.asarray(P["bbox_mean"], np.float32)), f32(np.asarray(P["bbox_std"], np.float32)), f32(im), f32(boxes)]
    src, dst = str(tmp_path / "model.bin"), str(tmp_path / "dets.bin")
    with open(src, "wb") as fh:
        fh.write(b"".join(blob))
    ex = os.path.join(ROOT, "examples", "c_host")
    r = subprocess.run(["make", "-C", ex], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    recs = {}
    for flag in ([], ["--augment"]):
        r = subprocess.run([os.path.join(ex, "frcnn_host")] + flag + [src, dst], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = open(dst, "rb").read()
        n = struct.unpack("<i", raw[:4])[0]
        recs[bool(flag)] = np.frombuffer(raw[4:], dtype=np.float32).reshape(n, 6)
    for flag in (False, True):
        net = models.FastRCNN(P, cfg=CFG, pooled=7, spatial_scale=1.0 / 16, max_h=H, max_w=W, max_rois=N, augment=flag)
        d, nd = net.test_one_async(_t(im, dev), _t(boxes, dev))
        torch.cuda.synchronize()
        py = d[: int(nd.item())].cpu().numpy()
        assert py.shape[0] > 0 and np.array_equal(recs[flag], py), flag
        net.close()
    assert not np.array_equal(recs[True], recs[False])
