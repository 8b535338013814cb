"""The integral loss on the plain Fast R-CNN handle (mpn_frcnn_create_integral, mpn_frcnn_train_set_head):
K classifiers in the fused head, scored by the mean of their softmaxes, trained one per minibatch.

Network, batches, the stale-rows recipe and THE YARDSTICK RULE (MARGIN = 2.0 beside PyTorch-CPU fp32 from the device's own pooled
operand) are tests/test_gpu_train.py's; the float64 side is tests/integral_np.py.  K = 3 goes with the head (fc 96, C 7) — a fused
head 49 wide, neither a multiple of 8 nor of 128 — and K = 6 with (fc 128, C 4) — 40 wide, a multiple of 8.  Apart from the K = 1
test the K classifiers are DIFFERENT matrices (_kparams), so reading or training the wrong head cannot pass.  Every
comparison with float64 prints its `ACC` line; the largest ratios measured on the MI355X are recorded in DESIGN.md section 13.7."""
import numpy as np
import pytest
import torch

import augment_np as A
import boxes_np as R
import integral_np as I
import test_gpu_train as G
import train_np as T

pytestmark = pytest.mark.gpu

KHEADS = [(3, (96, 7)), (6, (128, 4))]
KIDS = ["K%d_fc%d_C%d" % (k, h[0], h[1]) for k, h in KHEADS]
H, W, MAXR, MEAN, STD = G.H, G.W, G.MAXR, G.MEAN, G.STD
_bits, _t = G._bits, G._t


def _kparams(fc, C, K, distinct=True):
    """test_gpu_train's parameters with model_utils.integral's K clones of the classifier (models.integral_params).  distinct: clone 0
    stays what it is, clone k >= 1 is redrawn by models.rescale_heads at the SAME scale (head_scale "trained", seed 7001 + k) — K
    different classifiers, so that reading the wrong head shows in every forward result."""
    from multipathnet_amd import models
    P = G._params(fc, C)
    Q = models.integral_params(P, K)
    for k in range(1, K if distinct else 1):
        R_ = models.rescale_heads(P, "trained", seed=7001 + k)
        Q["cls_w"][k * C:(k + 1) * C] = R_["cls_w"]
        Q["cls_b"][k * C:(k + 1) * C] = R_["cls_b"]
    return Q


def _rows(K, k, C):
    sel = np.zeros(K * C, bool)
    sel[I.head_rows(K, k, C)] = True
    return sel


def _head_judgements(tag, K, k, C, Wd, P0, ref, P32, diff):
    """the yardstick rule over the eight tensors; diff: judge w_old - w (the gradient test) instead of w.  With k given the stacked
    classifier is judged on head k's rows alone (the others are checked bit for bit by the caller)."""
    bad = []
    for n in T.TENSORS:
        sel = _rows(K, k, C) if (k is not None and n in ("cls_w", "cls_b")) else slice(None)
        w_old = P0[n].astype(np.float64)[sel]
        r, r64, r32 = Wd[n][sel], ref.P[n][sel], P32[n][sel]
        if diff:
            r, r64, r32 = w_old - r, w_old - r64, w_old - r32
        ok, info = G._judge("%s %s" % (tag, n), r, r64, r32, w_new=Wd[n][sel])
        if not ok:
            bad.append(info)
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. K = 1 is the old handle
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", G.HEADS, ids=["fc%d_C%d" % h for h in G.HEADS])
def test_k1_is_the_handle_of_mpn_frcnn_create(dev, head):
    from multipathnet_amd import models
    fc, C = head
    P = G._params(fc, C)
    old, new = G._net(P), G._net(models.integral_params(P, 1))
    assert new.n_integral == 1 and old.n_integral == 1 and not new.noSoftMax
    assert new._lib.mpn_frcnn_n_integral(new._h) == 1 and old._lib.mpn_frcnn_n_integral(old._h) == 1
    out = []
    for net in (old, new):
        im, bx, s, b = G._stale(net, dev)
        net.train_begin(depth=2, momentum=0.9, weight_decay=5e-4, bbox_weight=1.0, dropout=0.5, seed=777)
        net.train_set_head(0)
        losses = []
        for i in range(2):
            G._add(net, dev, G._batch(5000 + i, 66 - 13 * i, C, 12))
            losses.append(net.train_step(1e-2))
        Wd = G._weights(net)
        net.train_end()
        s2, b2 = net.detect(im, bx)
        torch.cuda.synchronize()
        out.append((s.cpu().numpy(), b.cpu().numpy(), torch.stack(losses).cpu().numpy(), Wd, s2.cpu().numpy(), b2.cpu().numpy()))
    a, c = out
    assert _bits(a[0], c[0]) and _bits(a[1], c[1]), "detect differs between mpn_frcnn_create and mpn_frcnn_create_integral(.., 1)"
    assert _bits(a[2], c[2])
    for n in T.TENSORS:
        assert _bits(a[3][n], c[3][n]) and not _bits(a[3][n], G._np(P)[n]), n
    assert _bits(a[4], c[4]) and _bits(a[5], c[5]) and not _bits(a[0], a[4])


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. inference: the logits, the mean of the K softmaxes at the fused head's row pitch, the boxes
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("khead", KHEADS, ids=KIDS)
def test_inference_against_float64(dev, khead):
    K, (fc, C) = khead
    Q = _kparams(fc, C, K)
    Q0 = G._np(Q)
    net = G._net(Q)
    assert net.n_integral == K and net.noSoftMax and net.n_classes == C and net._lib.mpn_frcnn_n_integral(net._h) == K
    im, bx, s, b = G._stale(net, dev)
    s, b = s.cpu().numpy(), b.cpu().numpy()
    N = MAXR
    fc7 = net.debug_tensor("fc7", (N, fc)).cpu().numpy().astype(np.float64)
    cls_k = net.debug_tensor("cls_k", (N, K * C)).cpu().numpy()
    raw = net.debug_tensor("bbox_raw", (N, 4 * C)).cpu().numpy()
    # the K classifiers' logits against float64 from the device's own fc7: the head parity tests' bound on "cls" (absolute 1e-4)
    z64 = fc7 @ Q0["cls_w"].astype(np.float64).T + Q0["cls_b"].astype(np.float64)
    e = np.abs(cls_k - z64).max()
    print("ACC K%d cls_k vs float64 from the device's fc7: max|d| %.3g (bound 1e-4), logits %.3g .. %.3g" % (K, e, cls_k.min(), cls_k.max()))
    assert e < 1e-4
    # the scores against the float64 mean of softmaxes of the device's own logits: tests/test_gpu_box_kernels_numerics.py's bound
    ref = R.softmax_mean(cls_k.reshape(N, K, C))
    bound = R.softmax_bound(C, K)
    rel = np.abs(s.astype(np.float64) - ref) / np.maximum(ref, R.TINY)
    print("ACC K%d scores vs float64 softmax-mean of the device's cls_k: max rel %.3g (bound %.3g)" % (K, rel.max(), bound))
    assert (ref >= R.TINY).all() and (np.abs(s.astype(np.float64) - ref) <= bound * ref + 2.0 ** -125).all()
    one = R.softmax(cls_k.reshape(N, K, C)[:, 0])
    assert np.abs(ref - one).max() > 1e-3, "the K classifiers do not differ: the mean would not show a wrong row pitch"
    # the boxes: a K = 1 handle with the same bbox weights leaves the same bbox_raw and decodes it to the same boxes
    P1 = dict(Q)
    P1.pop("n_integral")
    P1["cls_w"], P1["cls_b"] = Q["cls_w"][:C].contiguous(), Q["cls_b"][:C].contiguous()
    net1 = G._net(P1)
    s1, b1 = net1.detect(im, bx)
    torch.cuda.synchronize()
    assert _bits(net1.debug_tensor("bbox_raw", (N, 4 * C)).cpu().numpy(), raw) and _bits(b1.cpu().numpy(), b)
    assert _bits(net1.debug_tensor("cls", (N, C)).cpu().numpy(), cls_k[:, :C])        # (and head 0's logits are that handle's)
    assert np.isfinite(b).all() and not _bits(s1.cpu().numpy(), s)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the other forms on a K = 3 handle
# ---------------------------------------------------------------------------------------------------------------------------------
def test_test_one_graphs_pipelined_and_cached_features(dev):
    K, (fc, C) = KHEADS[0]
    Q = _kparams(fc, C, K)
    off, on = G._net(Q), G._net(Q)
    off.set_graphs(False)
    on.set_graphs(True)
    im, bx, s, b = G._stale(off, dev)
    d0, n0 = off.test_one_async(im, bx)
    torch.cuda.synchronize()
    n0 = int(n0.item())
    d0 = d0[:n0].cpu().numpy().copy()
    assert n0 > 0
    for _ in range(4):   # captured at the second sighting of these buffers, replayed afterwards
        d, n = on.test_one_async(im, bx)
        torch.cuda.synchronize()
        assert int(n.item()) == n0 and np.array_equal(d[:n0].cpu().numpy(), d0, equal_nan=True)
    caps, reps = on.graph_stats()
    assert caps >= 1 and reps >= 1, (caps, reps)
    dp, np_ = off.test_one_pipelined(im, bx)   # the heads handed over to the side stream
    off.flush()
    torch.cuda.synchronize()
    assert int(np_.item()) == n0 and np.array_equal(dp[:n0].cpu().numpy(), d0, equal_nan=True)
    s2, b2 = off.detect(im, bx, recompute_features=False)
    assert torch.equal(s2, s) and torch.equal(b2, b)
    s3, b3 = off.detect(im, bx[:37].contiguous(), recompute_features=False)   # fewer rows: the same rows' bits
    assert torch.equal(s3, s[:37]) and torch.equal(b3, b[:37])


def test_flip_augmentation_is_the_merge_of_two_detects(O, dev):
    """tests/test_gpu_augment.py's statement for K = 1, on a K = 3 handle: detect == augment_np.merge of two plain detects, and what
    test_one keeps == the oracle's NMS / top-k on augment_np's tables"""
    K, (fc, C) = KHEADS[0]
    Q = _kparams(fc, C, K)
    plain, aug = G._net(Q), G._net(Q, augment=True)
    assert aug.augment and not plain.augment
    rng = np.random.default_rng(99)
    im, boxes = rng.random((3, H, W), dtype=np.float32), G._boxes(rng, MAXR)
    imd, imf, bd = _t(im, dev), _t(A.hflip(im), dev), _t(boxes, dev)

    def half(mirrored, bxs):
        sc_, bb_ = plain.detect(imf if mirrored else imd, _t(bxs, dev), clamp=False)
        torch.cuda.synchronize()
        return sc_.cpu().numpy(), bb_.cpu().numpy()
    sA, bA = half(False, boxes)
    sB, bB = half(True, A.flip_boxes(boxes, W))
    for clamp in (False, True):
        es, eb = A.merge(sA, bA, sB, bB, W, H, clamp=clamp)
        s, b = aug.detect(imd, bd, clamp=clamp)
        torch.cuda.synchronize()
        assert _bits(s.cpu().numpy(), es) and _bits(b.cpu().numpy(), eb), clamp
    assert not _bits(es, sA)
    dets, n = aug.test_one_async(imd, bd)
    torch.cuda.synchronize()
    dets = dets[: int(n.item())].cpu().numpy()
    keep, _, nk = [t.cpu().numpy() for t in aug.nms_results()]
    sc, bb = A.tester_tables(half, O.select_boxes, boxes, W, H, num_iter=1)
    per = []
    for j in range(1, C):
        sb, _ = O.select_scored(sc, bb, j, -1.5)
        ref = O.nms(sb, 0.3)
        assert nk[j - 1] == ref.shape[0] and np.array_equal(keep[j - 1, : nk[j - 1]], ref, equal_nan=True), j
        per.append(ref)
    kept, _ = O.keep_top_k(per, 100)
    exp = np.concatenate([np.concatenate([k_, np.full((k_.shape[0], 1), j + 1, np.float32)], 1) for j, k_ in enumerate(kept) if k_.size])
    assert dets.shape == exp.shape and dets.shape[0] > 0 and np.array_equal(dets, exp, equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the gradient: momentum 0, wd 0, lr 1, depth 2, one step on head k (test_gradient_against_float64 with a selector)
# ---------------------------------------------------------------------------------------------------------------------------------
GRAD_BATCHES = {"B70_two_images": [(33, 9), (37, 11)], "B1": [(1, 0)]}


@pytest.mark.parametrize("khead", KHEADS, ids=KIDS)
@pytest.mark.parametrize("last", [False, True], ids=["head0", "headK-1"])
@pytest.mark.parametrize("case", list(GRAD_BATCHES))
def test_gradient_against_float64(dev, khead, last, case):
    """The K classifiers here are model_utils.integral's own clones (the state of the first training step): the selected head's logits
    are then those of tests/test_gpu_train.py's gradient test, the computation MARGIN = 2.0 was measured on.  What lands where is
    checked by position — head k's rows move, every other classifier's rows keep their bits — and a forward pass that read the wrong
    head is caught where the heads differ (the inference test; the three-step test, whose losses are judged against float64).
    MEASURED with K DIFFERENT classifiers instead (MI355X, two choices of them): every tensor and the B = 70 losses stayed inside
    1.32, but the B = 1 loss pair read, over (K, head) = (3, 0), (3, 2), (6, 0), (6, 5): 0.00, 0.00, 0.70, 2.36 with clones scaled
    by 1 + 0.1 k plus noise, and 0.00, 0.00, 1.25, 5.73 with clones redrawn at the "trained" scale.  At B = 1 that ratio is one fp32
    rounding sample over another — two numbers a side, nothing averages: the device's error was 4.2e-7 and 1.8e-7 (about one ulp of
    the logits: the kernel's (mx + logf(sum)) - z[y] rounds at their magnitude), the yardstick's own 1.8e-7 and 3.2e-8.  The loss
    formula is the K = 1 kernel's and is not touched here (K = 1 keeps its bits); DESIGN.md section 13.7."""
    K, (fc, C) = khead
    k = K - 1 if last else 0
    Q = _kparams(fc, C, K, distinct=False)
    P0 = G._np(Q)
    net = G._net(Q)
    G._stale(net, dev)
    parts = [G._batch(1000 + 17 * i + fc, n, C, n_bg) for i, (n, n_bg) in enumerate(GRAD_BATCHES[case])]
    if case == "B1":
        parts = [tuple(a[1:2] if j else a for j, a in enumerate(G._batch(1234, 2, C, 0)))]
    net.train_begin(depth=2, momentum=0.0, weight_decay=0.0, bbox_weight=1.0)
    G._add(net, dev, G._batch(77, MAXR, C, 60))
    net.train_step(0.0)   # max_rois rows at lr 0 on head 0: the minibatch's own buffers now hold stale rows too
    assert all(_bits(v, P0[n]) for n, v in G._weights(net).items())
    for b in parts:
        G._add(net, dev, b)
    net.train_set_head(k)   # with the rows pending: the head is read at the step
    loss = net.train_step(1.0).cpu().numpy()
    rois, gt, labels = G._join(parts)
    B = len(labels)
    x = G._pooled(net, B)
    Wd = G._weights(net)
    net.train_end()
    # every unselected classifier: not one bit moved
    other = ~_rows(K, k, C)
    assert _bits(Wd["cls_w"][other], P0["cls_w"][other]) and _bits(Wd["cls_b"][other], P0["cls_b"][other]), "an unselected classifier changed"
    assert not _bits(Wd["cls_w"][~other], P0["cls_w"][~other])
    ref = I.Sgd64(P0, K, depth=2, momentum=0.0, weight_decay=0.0, mean=MEAN, std=STD)
    l64, d = ref.step(x, rois, gt, labels, lr=1.0, k=k)
    if B > 1:
        assert (np.abs(d) < 1).any() and (np.abs(d) >= 1).any() and (labels == 0).any() and (labels > 0).any()
    P32, l32 = I.torch_steps(P0, [(x, rois, gt, labels)], [k], 1.0, K, depth=2, momentum=0.0, weight_decay=0.0, mean=MEAN, std=STD, dtype=torch.float32)
    bad = _head_judgements("K%d k%d %s" % (K, k, case), K, k, C, Wd, P0, ref, P32, diff=True)
    ok, info = G._judge("K%d k%d %s loss" % (K, k, case), loss, np.array(l64), np.array(l32[0], np.float32), w_new=loss)
    if not ok:
        bad.append(info)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the unselected heads are stepped: heads 0, 1, 2 in turn with momentum and weight decay
# ---------------------------------------------------------------------------------------------------------------------------------
def _steps(net, dev, C, schedule, lr=1e-3, seed0=2000, first=0):
    """steps first .. len(schedule) - 1 of the schedule, a new (shrinking) batch each; -> (batches with the device's pooled operand, losses)"""
    batches, losses = [], []
    for i in range(first, len(schedule)):
        b = G._batch(seed0 + i, 66 - 11 * i, C, 12)
        G._add(net, dev, b)
        net.train_set_head(schedule[i])
        losses.append(net.train_step(lr))
        batches.append((G._pooled(net, len(b[3])), b[1], b[2], b[3]))
    return batches, torch.stack(losses).cpu().numpy()


@pytest.mark.parametrize("khead", KHEADS, ids=KIDS)
def test_three_steps_heads_in_turn_against_float64(dev, khead):
    K, (fc, C) = khead
    Q = _kparams(fc, C, K)
    P0 = G._np(Q)
    net = G._net(Q)
    G._stale(net, dev)
    net.train_begin(depth=2, momentum=0.9, weight_decay=5e-4, bbox_weight=1.0)
    batches, losses = _steps(net, dev, C, [0, 1, 2])
    Wd = G._weights(net)
    net.train_end()
    ref = I.Sgd64(P0, K, depth=2, momentum=0.9, weight_decay=5e-4, mean=MEAN, std=STD)
    l64 = [ref.step(*b, lr=1e-3, k=k)[0] for k, b in enumerate(batches)]
    P32, l32 = I.torch_steps(P0, batches, [0, 1, 2], 1e-3, K, depth=2, momentum=0.9, weight_decay=5e-4, mean=MEAN, std=STD, dtype=torch.float32)
    bad = _head_judgements("K%d heads 0,1,2" % K, K, None, C, Wd, P0, ref, P32, diff=False)
    ok, info = G._judge("K%d heads 0,1,2 losses" % K, losses, np.array(l64), np.array(l32, np.float32), w_new=losses)
    if not ok:
        bad.append(info)
    assert not bad, bad
    # an unselected classifier is stepped: the decay and its momentum moved every head's weights, also in the steps that trained another
    for k in range(K):
        sel = _rows(K, k, C)
        assert not _bits(Wd["cls_w"][sel], P0["cls_w"][sel]), "classifier %d did not move" % k
    if K > 3:   # never selected: zero gradient all along — the weights decayed (float64 says by how much), the biases (no decay) kept their bits
        never = np.zeros(K * C, bool)
        never[3 * C:] = True
        assert _bits(Wd["cls_b"][never], P0["cls_b"][never])
        assert np.abs(Wd["cls_w"][never] - ref.P["cls_w"][never]).max() <= 4 * G.U * np.abs(P0["cls_w"][never]).max()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. determinism and resume with dropout; 7. in place
# ---------------------------------------------------------------------------------------------------------------------------------
def test_determinism_resume_and_in_place_update(dev, tmp_path):
    from multipathnet_amd import train
    K, (fc, C) = KHEADS[0]
    Q = _kparams(fc, C, K)
    schedule = [0, 1, 2, 1]
    kw = dict(depth=2, momentum=0.9, weight_decay=5e-4, bbox_weight=1.0, dropout=0.5, seed=4242)

    def run(stop=None):
        net = G._net(Q)
        im, bx, _, _ = G._stale(net, dev)
        net.train_begin(**kw)
        _, losses = _steps(net, dev, C, schedule[:stop] if stop else schedule, lr=1e-2)
        return net, losses, im, bx
    a, la, im, bx = run()
    Wa = G._weights(a)
    b, lb, _, _ = run()
    Wb = G._weights(b)
    b.train_end()
    assert _bits(la, lb) and all(_bits(Wa[n], Wb[n]) for n in T.TENSORS), "the same schedule twice gave different bits"
    assert not any(_bits(Wa[n], G._np(Q)[n]) for n in T.TENSORS)
    # stop after step 2, through one .t7 file, a new handle, the rest of the same schedule
    c, lc, _, _ = run(stop=2)
    path = str(tmp_path / "ckpt_integral.t7")
    train.save_checkpoint(path, c)
    c.train_end()
    ck = train.load_checkpoint(path)
    assert ck["weights"]["n_integral"] == K and ck["weights"]["cls_w"].shape == (K * C, fc) and ck["state"]["cls_w"].shape == (K * C, fc)
    assert ck["state"]["step"] == 2 and ck["dropout"] == 0.5 and ck["seed"] == 4242
    Pn = dict(Q)
    Pn.update(ck["weights"])
    d = G._net(Pn)
    assert d.n_integral == K
    G._stale(d, dev)
    d.train_begin(**kw)
    train.resume(d, ck)
    _, ld = _steps(d, dev, C, schedule, lr=1e-2, first=2)
    Wd = G._weights(d)
    d.train_end()
    assert _bits(np.concatenate([lc, ld]), la), "the resumed run's losses differ from the uninterrupted run's"
    for n in T.TENSORS:
        assert _bits(Wd[n], Wa[n]), "resumed run: %s differs from the uninterrupted run" % n
    # 7. in place: detect on the trained handle == detect on a fresh handle created from its head_weights()
    s1, b1 = a.detect(im, bx)
    W1 = a.head_weights()
    assert W1["cls_w"].shape == (K * C, fc) and W1["cls_b"].shape == (K * C,)
    St = a.train_state()
    assert St["cls_w"].shape == (K * C, fc) and St["cls_b"].shape == (K * C,) and St["step"] == 4
    a.train_end()
    Pf = dict(Q)
    Pf.update({n: v.cpu() for n, v in W1.items()})
    fresh = G._net(Pf)
    s2, b2 = fresh.detect(im, bx)
    torch.cuda.synchronize()
    assert _bits(s1.cpu().numpy(), s2.cpu().numpy()) and _bits(b1.cpu().numpy(), b2.cpu().numpy())
    W2 = G._weights(fresh)   # unpack -> create -> unpack
    for n in T.TENSORS:
        assert _bits(W1[n].cpu().numpy(), W2[n]), n


def test_a_k1_checkpoint_has_no_integral_key(dev, tmp_path):
    from multipathnet_amd import t7, train
    fc, C = G.HEADS[1]
    net = G._net(G._params(fc, C))
    net.train_begin(depth=0)
    path = str(tmp_path / "ckpt_k1.t7")
    train.save_checkpoint(path, net)
    net.train_end()
    assert "n_integral" not in t7.load(path) and "n_integral" not in train.load_checkpoint(path)["weights"]


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from multipathnet_amd import MpnError, parallel
    K, (fc, C) = KHEADS[0]
    net = G._net(_kparams(fc, C, K))
    im, bx, s0, b0 = G._stale(net, dev)

    def refused(call, status, *words):
        with pytest.raises(MpnError) as ei:
            call()
        assert "status %d" % status in str(ei.value) and all(w in str(ei.value) for w in words), str(ei.value)
    refused(lambda: net.train_set_head(0), -5, "mpn_frcnn_train_begin")             # before train_begin: MPN_ESTATE
    net.train_begin(depth=0)
    refused(lambda: net.train_set_head(K), -1, "K = %d" % K)                        # MPN_EINVAL, naming K
    refused(lambda: net.train_set_head(-1), -1, "K = %d" % K)
    net.train_set_head(K - 1)
    net.train_end()
    refused(lambda: net.train_set_head(0), -5)
    # the sharded forms cut the head by class: MPN_ESTATE, naming the reason
    rows_f, cls_f = net.shard_record_floats(MAXR, 1)
    z = lambda n: torch.zeros(max(n, 1), dtype=torch.float32, device=dev)
    refused(lambda: net.shard_head(im, bx, 0, 1), -5, "integral")
    refused(lambda: net.shard_nms(z(rows_f), MAXR, 0, 1), -5, "integral")
    refused(lambda: net.shard_finish(z(cls_f), MAXR, 1), -5, "integral")
    comm = parallel.Comm.single(use_rccl=False)
    try:
        refused(lambda: net.test_one_sharded(comm, im, bx), -5, "integral")
    finally:
        comm.close()
    refused(lambda: net.debug_tensor("cls", (MAXR, C)), -1, "cls_k")                # MPN_EINVAL, naming "cls_k"
    # a K = 1 handle takes head 0 only; and the K = 3 handle still works after all the refusals
    one = G._net(G._params(fc, C))
    one.train_begin(depth=0)
    one.train_set_head(0)
    refused(lambda: one.train_set_head(1), -1, "K = 1")
    one.train_end()
    s1, b1 = net.detect(im, bx)
    assert torch.equal(s1, s0) and torch.equal(b1, b0)
