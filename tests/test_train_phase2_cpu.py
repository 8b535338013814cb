"""tests/train_phase2_np.py checked on the CPU: the autograd step with given routing against the one that
routes itself, nn.Normalize's closed-form backward against autograd, the two fp32 restatements against the bounds
tests/test_gpu_train_phase2.py uses, the device-free refusals of the new entry points, and the edge cases the GPU file's inputs hold."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_conv_np as TC  # noqa: E402
import train_phase2_np as P2  # noqa: E402
import train_towers_np as TT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def _small(seed=3, c_in=5, chans=(8, 6, 8), h=9, w=12, fc=16, Cn=4, K=2, n_rows=(5, 4)):
    """a small phase-2 problem: a three-layer block on two images' input maps, five towers on c5 = 8 channels (+ 3 / + 5 constant columns)"""
    rng = np.random.default_rng(seed)
    c5 = chans[-1]
    conv, cin = {}, c_in
    for j, co in enumerate(chans):
        conv[7 + j] = (rng.normal(0, (2.0 / (9 * cin)) ** 0.5, (co, cin, 3, 3)), rng.normal(0, 0.1, co))
        cin = co
    extra = [8, 3, 3, 0, 8]
    P = {}
    for t in range(5):
        kc = c5 + extra[t]
        P["t%d.mix_w" % t], P["t%d.mix_b" % t] = rng.normal(0, 0.02, (c5, kc)), rng.normal(0, 0.01, c5)
        P["t%d.fc6_w" % t], P["t%d.fc6_b" % t] = rng.normal(0, 0.05, (fc, c5 * 49)), rng.normal(0, 0.01, fc)
        P["t%d.fc7_w" % t], P["t%d.fc7_b" % t] = rng.normal(0, 0.2, (fc, fc)), rng.normal(0, 0.01, fc)
    P["cls_w"], P["cls_b"] = rng.normal(0, 0.1, (K * Cn, 4 * fc)), np.zeros(K * Cn)
    P["bbox_w"], P["bbox_b"] = rng.normal(0, 0.05, (4 * Cn, fc)), np.zeros(4 * Cn)
    images, rois, gt, labels = [], [], [], []
    for n in n_rows:
        a0 = np.abs(rng.normal(0, 1, (c_in, h, w)))
        ctr = rng.uniform([40, 40], [16 * w - 40, 16 * h - 40], (n, 2))
        wh = rng.uniform(30, 70, (n, 2))
        bx = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(np.float32)
        images.append((a0, P2.foveal(P2.project(bx))))
        rois.append(bx)
        gt.append(bx + rng.normal(0, 1.0, (n, 4)).astype(np.float32))
        labels.append(rng.integers(1, Cn, n))
    labels[0][0] = 0
    B = sum(n_rows)
    rest = [rng.normal(0, 5, (B, extra[t], 49)) for t in range(5)]
    return P, conv, images, rest, np.concatenate(rois), np.concatenate(gt), np.concatenate(labels), K


def test_given_routing_equals_own_routing_in_float64():
    P, conv, images, rest, rois, gt, labels, K = _small()
    mk = lambda: P2.Trainer(P, conv, K, 0.0, 0.0, mean=P2.MEAN, std=P2.STD, dtype=torch.float64)
    own = mk()
    _, G_own = own.step([(a0, None, None, fov) for a0, fov in images], P2.REGIONS, rest, rois, gt, labels, 1.0, k=1)
    # the routing the own run took, computed apart: the masks of every layer's output and the first maximum of every Foveal window
    probe, given = mk(), []
    for a0, fov in images:
        a = torch.as_tensor(a0)[None]
        masks = []
        for l in probe.layers:
            a = torch.relu(torch.nn.functional.conv2d(a, probe.Pt["conv_w.%d" % l].detach(), probe.Pt["conv_b.%d" % l].detach(), padding=1))
            masks.append(a[0].numpy() > 0)
        top = a[0].numpy()
        am = {r: TC.own_argmax(top, fov[:, r], 7, 7, P2.SCALE) for r in set(P2.REGIONS)}
        for r in am:   # no positive tie: the maximum of every window that has a positive one is unique
            for n, row in enumerate(TC.roi_windows(fov[:, r], top.shape[1], top.shape[2], 7, 7, P2.SCALE)):
                for b, (hs, he, ws, we) in enumerate(row):
                    if he > hs and we > ws:
                        sub = top[:, hs:he, ws:we].reshape(top.shape[0], -1)
                        mx = sub.max(1)
                        assert ((sub == mx[:, None]).sum(1)[mx > 0] == 1).all()
        given.append((a0, masks, am, fov))
    giv = mk()
    _, G_giv = giv.step(given, P2.REGIONS, rest, rois, gt, labels, 1.0, k=1)
    for n in G_own:
        assert np.abs(G_own[n]).max() > 0 or n.startswith("cls") , n
        np.testing.assert_allclose(G_giv[n], G_own[n], rtol=1e-11, atol=1e-13 * max(np.abs(G_own[n]).max(), 1e-30), err_msg=n)
    for n in P2.conv_names(own.layers):
        assert np.abs(G_own[n]).max() > 0, n


def test_normalize_closed_form_is_autograd_in_float64():
    rng = np.random.default_rng(5)
    x = np.abs(rng.normal(0, 1, (6, 16, 49)))
    x[1] = 0.0            # an all-zero row: the 1e-10 inside the root decides
    x[2, :, 10:] = 0.0
    g = rng.normal(0, 1, x.shape)
    xt = torch.as_tensor(x).requires_grad_(True)
    yt = xt / torch.sqrt((xt * xt).sum((1, 2), keepdim=True) + 1e-10) * P2.MUL
    yt.backward(torch.as_tensor(g))
    got = P2.normalize_backward64(x, yt.detach().numpy(), g)
    ref = xt.grad.numpy()
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.abs(ref[1]).max() > 0   # at x = 0 the Jacobian is (mul / 1e-5) I: the gradient passes, scaled


def test_fp32_normalize_backward_meets_its_bound():
    rng = np.random.default_rng(6)
    for c5, PP, scale in ((48, 49, 1.0), (64, 49, 30.0), (8, 4, 1e-3), (48, 49, 0.0)):
        x = (np.abs(rng.normal(0, 1, (7, c5, PP))) * (rng.random((7, c5, PP)) > 0.4) * scale).astype(np.float32)
        s32 = (np.float32(P2.MUL) / np.sqrt((x.astype(np.float64) ** 2).sum((1, 2)) + 1e-10)).astype(np.float32)
        y = (x * s32[:, None, None]).astype(np.float32)   # the stored operand: an fp32 product with an fp32 scale
        g = rng.normal(0, 1e-3, x.shape).astype(np.float32)
        got = P2.normalize_backward_f32(x, y, g)
        err = np.abs(got.astype(np.float64) - P2.normalize_backward64(x, y, g))
        bound = P2.normalize_backward_bound(x, y, g)
        assert (err <= bound).all(), (c5, PP, scale, float((err / np.maximum(bound, 1e-300)).max()))
        if scale:
            assert err.max() > 0 and (bound <= 64 * U * np.abs(got).max() + 1e-30).all()   # the bound is a few dozen ulps of the largest entry, not slack


def test_fp32_gradient_chain_is_the_ordered_sum():
    rng = np.random.default_rng(8)
    c5, h, w, B = 8, 6, 7, 9
    top = (rng.normal(0, 1, (c5, h, w)) * (rng.random((c5, h, w)) > 0.3)).clip(0).astype(np.float32)
    am = {r: rng.integers(-1, h * w, (B, c5, 49)) for r in set(P2.REGIONS)}
    dx = [rng.normal(0, 1, (B, c5, 49)).astype(np.float32) for _ in P2.REGIONS]
    got = P2.g5_chain(dx, am, P2.REGIONS, 2, 5, top)
    ref, mag = np.zeros((c5, h * w)), np.zeros((c5, h * w))
    n_terms = np.zeros((c5, h * w))
    ch = np.broadcast_to(np.arange(c5)[None, :, None], (5, c5, 49))
    for t, r in enumerate(P2.REGIONS):
        i = am[r][2:7]
        ok = i >= 0
        np.add.at(ref, (ch[ok], i[ok]), dx[t][2:7][ok].astype(np.float64))
        np.add.at(mag, (ch[ok], i[ok]), np.abs(dx[t][2:7][ok]).astype(np.float64))
        np.add.at(n_terms, (ch[ok], i[ok]), 1.0)
    mask = top.reshape(c5, -1) > 0
    ref = np.where(mask, ref, 0.0)
    assert n_terms.max() >= 3 and (got.reshape(c5, -1)[~mask] == 0).all()
    assert (np.abs(got.reshape(c5, -1) - ref) <= n_terms * U * mag + 1e-300).all()   # a chain of n adds: at most n roundings of partial sums <= the sum of magnitudes
    # the order is the contract's: towers ascending — the terms of towers 1 and 4 (one region, one argmax) are not adjacent
    one = np.zeros_like(dx[0])
    big = [one.copy() for _ in P2.REGIONS]
    cell = {r: np.full((B, c5, 49), -1, np.int64) for r in am}
    cell[1][2, 0, 0], cell[0][2, 0, 0] = 3, 3
    big[0][2, 0, 0], big[1][2, 0, 0], big[4][2, 0, 0] = np.float32(1.0), np.float32(2.0 ** 24), np.float32(-2.0 ** 24)
    t1 = np.ones((c5, h, w), np.float32)
    assert P2.g5_chain(big, cell, P2.REGIONS, 2, 1, t1)[0].reshape(-1)[3] == 0.0   # ((1 + 2^24) - 2^24 in tower order: the 1 is lost
    big[0][2, 0, 0], big[4][2, 0, 0] = np.float32(-2.0 ** 24), np.float32(1.0)
    assert P2.g5_chain(big, cell, P2.REGIONS, 2, 1, t1)[0].reshape(-1)[3] == 1.0   # (-2^24 + 2^24) + 1


def test_inputs_hold_the_required_edge_cases():
    """the boxes of tests/test_gpu_train_phase2.py's two-image gradient case on network C's 10 x 16 conv5 map"""
    c = P2.NETS["C"]
    parts = P2.grad_parts("C", "B70_two_images")
    h, w = P2.map_size(c["cfg"], 9)
    assert (h, w) == (10, 16)
    empty = two_towers = two_rows = False
    for p in parts:
        fov = P2.foveal(P2.project(p[1]))
        cover = []   # per tower: how many of the image's rows have a bin window over each cell
        for r in P2.REGIONS:
            cnt = np.zeros((h, w), int)
            for row in TC.roi_windows(fov[:, r], h, w, 7, 7, P2.SCALE):
                hit = np.zeros((h, w), bool)
                for hs, he, ws, we in row:
                    if he <= hs or we <= ws:
                        empty = True
                    hit[hs:he, ws:we] = True
                cnt += hit
            cover.append(cnt)
        two_rows = two_rows or any((cv >= 2).any() for cv in cover)
        two_towers = two_towers or bool((sum((cv > 0).astype(int) for cv in cover) >= 2).any())
    assert empty, "no Foveal region is clipped off the map: no empty bin"
    assert two_towers and two_rows
    # the first-maximum tie: a bin over several cells that are all 0.  On the CPU: network C's trunk on the case's first image, in
    # fp32 by PyTorch; a cell counts as 0 only where its pre-activation is below -1e-3, far from any rounding of the device's convolution
    P = P2.params("C")
    im = torch.as_tensor(parts[0][0])
    a = (im[[2, 1, 0]] * 255.0 - torch.tensor([102.9801, 115.9465, 122.7717])[:, None, None])[None]
    li = 0
    for item in c["cfg"]:
        if item == "P":
            a = torch.nn.functional.max_pool2d(a, 2, 2, ceil_mode=True)
        else:
            pre = torch.nn.functional.conv2d(a, P["conv_w"][li].float(), P["conv_b"][li].float(), padding=1)
            a, li = torch.relu(pre), li + 1
    dead = (pre[0] < -1e-3).numpy()
    fov = P2.foveal(P2.project(parts[0][1]))
    tie = False
    for r in set(P2.REGIONS):
        for row in TC.roi_windows(fov[:, r], h, w, 7, 7, P2.SCALE):
            for hs, he, ws, we in row:
                if (he - hs) * (we - ws) >= 2 and he > hs and we > ws:
                    tie = tie or bool(dead[:, hs:he, ws:we].reshape(dead.shape[0], -1).all(1).any())
    assert tie, "no bin of several cells is all zero in some channel: the first-maximum tie is not in the inputs"


def _lib():
    import multipathnet_amd
    lib = multipathnet_amd.load()
    lib.mpn_last_error.restype = C.c_char_p
    return lib


def test_refusals_without_a_device_come_from_the_product_library():
    lib = _lib()
    assert lib.mpn_version() == 600
    f = C.c_float
    assert lib.mpn_mpnet_train_begin_conv(None, 1, f(0.9), f(5e-4), f(1.0)) == -1 and b"mpn_mpnet_train_begin_conv" in lib.mpn_last_error()
    assert lib.mpn_mpnet_get_trunk_weights(None, 0, None, None, None) == -1 and b"mpn_mpnet_get_trunk_weights" in lib.mpn_last_error()
    assert lib.mpn_mpnet_train_get_trunk_state(None, 0, None, None, None) == -1 and b"mpn_mpnet_train_get_trunk_state" in lib.mpn_last_error()
    assert lib.mpn_mpnet_train_set_trunk_state(None, 0, None, None, None) == -1 and b"mpn_mpnet_train_set_trunk_state" in lib.mpn_last_error()


def test_header_and_cdef_declare_the_entries_and_keep_the_version():
    h = open(os.path.join(ROOT, "include", "mpn.h")).read()
    assert re.search(r"#define\s+MPN_VERSION\s+600\b", h)
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_lua_cdef.py"), "--check"]) == 0
    cdef = open(os.path.join(ROOT, "multipathnet_amd", "lua", "mpn_cdef.lua")).read()
    for proto in ("int mpn_mpnet_train_begin_conv(mpn_frcnn *p, int conv_layers, float momentum, float weight_decay, float bbox_weight);",
                  "int mpn_mpnet_get_trunk_weights(mpn_frcnn *p, int layer,", "int mpn_mpnet_train_get_trunk_state(mpn_frcnn *p, int layer,",
                  "int mpn_mpnet_train_set_trunk_state(mpn_frcnn *p, int layer, const float *d_v, const float *d_vb, void *stream);"):
        assert proto in h and proto in cdef, proto


def test_checkpoint_table_carries_conv_layers_and_old_files_load_as_zero():
    from multipathnet_amd import train
    rng = np.random.default_rng(2)
    a = lambda *s: rng.normal(0, 1, s).astype(np.float32)
    tow = [dict(mix_w=a(4, 6), mix_b=a(4), fc6_w=a(3, 16), fc6_b=a(3), fc7_w=a(3, 3), fc7_b=a(3), region=t % 4, use4=1, use3=0) for t in range(2)]
    Wt = dict(towers=tow, cls_w=a(4, 3), cls_b=a(4), bbox_w=a(8, 3), bbox_b=a(8), n_integral=2, n_classes=2, conv_w=[a(2, 3, 3, 3), a(4, 2, 3, 3)],
              conv_b=[a(2), a(4)])
    st = dict(towers=[{k: a(*np.shape(T[k])) for k in ("mix_w", "mix_b", "fc6_w", "fc6_b", "fc7_w", "fc7_b")} for T in tow], cls_w=a(4, 3), cls_b=a(4),
              bbox_w=a(8, 3), bbox_b=a(8), step=5)
    old = train.checkpoint_read(train.mpnet_checkpoint_table(Wt, st, 0.5, 7))
    assert old["conv_layers"] == 0 and "conv_w" not in old["state"]
    assert "conv_layers" not in train.mpnet_checkpoint_table(Wt, st, 0.5, 7)   # a phase-1 file is what it was
    st2 = dict(st, conv_w=[None, a(4, 2, 3, 3)], conv_b=[None, a(4)])
    new = train.checkpoint_read(train.mpnet_checkpoint_table(Wt, st2, 0.5, 7))
    assert new["conv_layers"] == 1 and new["state"]["conv_w"][0] is None
    assert np.array_equal(new["state"]["conv_w"][1].numpy(), st2["conv_w"][1]) and np.array_equal(new["state"]["conv_b"][1].numpy(), st2["conv_b"][1])
