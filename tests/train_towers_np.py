"""Float64 restatement of one training step of MultiPathNet's towers with the trunk frozen (test infrastructure; include/mpn.h
mpn_mpnet_train_*; models/multipathnet.lua phase 1).  Everything starts from the towers' operands
x_t [B, Kcat_t, PP] — the normalised ROI pools of tower t's maps side by side, Torch order — so the frozen trunk, the pooling and
nn.Normalize are no part of it:
    m_t  = x_t Wmix_t^T + bmix_t per bin  -> [B, c5 * PP], channel-major then bin (fc6's K order); NO ReLU behind it
    y6_t = relu(m_t W6_t^T + b6_t) * d6_t,   y7_t = relu(y6_t W7_t^T + b7_t) * d7_t      (d: the dropout multipliers, 1 without)
    cat  = [y7_0 | .. | y7_{T-1}],  z = cat[:, :(T-1)F] Wcls^T + bcls  [B, K*C],  t^ = cat[:, (T-1)F:] Wbbox^T + bbbox  [B, 4C]
    loss: tests/train_np.py's on classifier k's columns of z and on t^ (1/B, bbox_weight/B); optim.sgd as train_np.Sgd64.
Parameters are a flat dict: "t<i>.mix_w" [c5, Kcat_i], "t<i>.mix_b", "t<i>.fc6_w" [F, c5*PP], "t<i>.fc6_b", "t<i>.fc7_w", "t<i>.fc7_b",
"cls_w" [K*C, (T-1)F], "cls_b", "bbox_w" [4C, F], "bbox_b" (flat() makes it from synthetic_mpnet_params' shape).

torch_steps is the same computation by PyTorch-CPU autograd + torch.optim.SGD in a chosen dtype: in float64 it checks this file
(tests/test_train_towers_cpu.py), in float32 it is the yardstick the device is judged against (tests/test_gpu_train_towers.py)."""
import numpy as np

import dropout_np as D
import train_np as T

TOWER_TENSORS = ("mix_w", "mix_b", "fc6_w", "fc6_b", "fc7_w", "fc7_b")
HEAD_TENSORS = ("cls_w", "cls_b", "bbox_w", "bbox_b")


def names(n_towers):
    return ["t%d.%s" % (t, k) for t in range(n_towers) for k in TOWER_TENSORS] + list(HEAD_TENSORS)


def is_weight(name):
    return name.endswith("_w")


def flat(P):
    """synthetic_mpnet_params' shape (or tower_weights()') -> the flat dict of numpy arrays"""
    a = lambda v: np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v)
    out = {"t%d.%s" % (t, k): a(W[k]) for t, W in enumerate(P["towers"]) for k in TOWER_TENSORS}
    out.update({k: a(P[k]) for k in HEAD_TENSORS})
    return out


def n_towers_of(P):
    return sum(1 for k in P if k.endswith(".mix_w"))


def masks(seed, step, n_towers, B, F, rate):
    """[(d6_t, d7_t)] float32 multipliers [B, F]: tower t's layers are 2t (behind fc6) and 2t + 1 (behind fc7) of dropout_np's stream"""
    if not rate:
        one = np.ones((B, F), np.float32)
        return [(one, one)] * n_towers
    s = D.scale(rate)
    mk = lambda layer: np.where(D.keep_mask(seed, step, layer, B, F, rate), s, np.float32(0)).astype(np.float32)
    return [(mk(2 * t), mk(2 * t + 1)) for t in range(n_towers)]


def forward(P, xs, drop):
    """-> per tower (m, a6, y6, a7, y7), cat, z, t^"""
    nt = len(xs)
    tow = []
    for t in range(nt):
        x = xs[t]                                                       # [B, Kcat, PP]
        m = np.einsum("bkp,nk->bnp", x, P["t%d.mix_w" % t]) + P["t%d.mix_b" % t][None, :, None]
        m = m.reshape(x.shape[0], -1)
        a6 = m @ P["t%d.fc6_w" % t].T + P["t%d.fc6_b" % t]
        y6 = np.maximum(a6, 0.0) * drop[t][0]
        a7 = y6 @ P["t%d.fc7_w" % t].T + P["t%d.fc7_b" % t]
        y7 = np.maximum(a7, 0.0) * drop[t][1]
        tow.append((m, a6, y6, a7, y7))
    cat = np.concatenate([w[4] for w in tow], 1)
    F = tow[0][4].shape[1]
    z = cat[:, :(nt - 1) * F] @ P["cls_w"].T + P["cls_b"]
    that = cat[:, (nt - 1) * F:] @ P["bbox_w"].T + P["bbox_b"]
    return tow, cat, z, that


def loss_and_grads(P, xs, rois, gt, labels, K, k, mean, std, bbox_weight=1.0, drop=None):
    """-> ((L_cls, L_box), {name: gradient}, d [n_fg, 4] the smooth-L1 arguments, gz [B, K*C] the gradient at z)"""
    nt = len(xs)
    P = {n: np.asarray(P[n], np.float64) for n in names(nt)}
    xs = [np.asarray(x, np.float64) for x in xs]
    labels = np.asarray(labels, np.int64)
    B = xs[0].shape[0]
    C = P["bbox_w"].shape[0] // 4
    F = P["bbox_w"].shape[1]
    assert P["cls_w"].shape[0] == K * C and 0 <= k < K
    drop = [(np.asarray(a, np.float64), np.asarray(b, np.float64)) for a, b in (drop or masks(0, 0, nt, B, F, 0.0))]
    tow, cat, z, that = forward(P, xs, drop)
    zk = z[:, k * C:(k + 1) * C]
    mx = zk.max(1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(zk - mx).sum(1))
    L_cls = float((lse - zk[np.arange(B), labels]).sum() / B)
    gk = np.exp(zk - lse[:, None])
    gk[np.arange(B), labels] -= 1.0
    gz = np.zeros_like(z)
    gz[:, k * C:(k + 1) * C] = gk / B
    t, fg = T.targets(rois, gt, labels, mean, std)
    gt_hat = np.zeros_like(that)
    idx = np.nonzero(fg)[0]
    cols = 4 * labels[idx][:, None] + np.arange(4)[None, :]
    d = that[idx[:, None], cols] - t[idx]
    L_box = float(bbox_weight * np.where(np.abs(d) < 1.0, 0.5 * d * d, np.abs(d) - 0.5).sum() / B)
    gt_hat[idx[:, None], cols] = bbox_weight / B * np.clip(d, -1.0, 1.0)
    nf = nt - 1
    G = {"cls_w": gz.T @ cat[:, :nf * F], "cls_b": gz.sum(0), "bbox_w": gt_hat.T @ cat[:, nf * F:], "bbox_b": gt_hat.sum(0)}
    dcat = np.concatenate([gz @ P["cls_w"], gt_hat @ P["bbox_w"]], 1)
    for i in range(nt):
        m, a6, y6, a7, y7 = tow[i]
        g7 = dcat[:, i * F:(i + 1) * F] * drop[i][1] * (a7 > 0)
        G["t%d.fc7_w" % i], G["t%d.fc7_b" % i] = g7.T @ y6, g7.sum(0)
        g6 = (g7 @ P["t%d.fc7_w" % i]) * drop[i][0] * (a6 > 0)
        G["t%d.fc6_w" % i], G["t%d.fc6_b" % i] = g6.T @ m, g6.sum(0)
        gm = (g6 @ P["t%d.fc6_w" % i]).reshape(B, -1, xs[i].shape[2])   # unmasked: [B, c5, PP]
        G["t%d.mix_w" % i], G["t%d.mix_b" % i] = np.einsum("bnp,bkp->nk", gm, xs[i]), gm.sum((0, 2))
    return (L_cls, L_box), G, d, gz


class Sgd64(object):
    """optim.sgd over every tower and head tensor in float64: g += wd * w for weights only, v = momentum * v + g, w -= lr * v"""

    def __init__(self, P, K, momentum=0.9, weight_decay=5e-4, bbox_weight=1.0, mean=None, std=None):
        self.nt = n_towers_of(P)
        self.P = {n: np.array(np.asarray(P[n]), np.float64) for n in names(self.nt)}
        self.V = {n: np.zeros_like(self.P[n]) for n in self.P}
        self.K, self.momentum, self.wd, self.bbox_weight, self.mean, self.std = K, momentum, weight_decay, bbox_weight, mean, std

    def step(self, xs, rois, gt, labels, lr, k=0, drop=None):
        loss, G, d, gz = loss_and_grads(self.P, xs, rois, gt, labels, self.K, k, self.mean, self.std, self.bbox_weight, drop)
        for n in self.P:
            g = G[n] + (self.wd * self.P[n] if is_weight(n) else 0.0)
            self.V[n] = self.momentum * self.V[n] + g
            self.P[n] = self.P[n] - lr * self.V[n]
        return loss, d, gz


def torch_steps(P, batches, lr, K, momentum=0.9, weight_decay=5e-4, bbox_weight=1.0, mean=None, std=None, dtype=None):
    """The same steps by PyTorch-CPU: batches [(xs, rois, gt, labels, k, drop or None)], the multipliers constants of the graph; every
    classifier is in the optimiser, so the ones not selected see weight decay and momentum with a zero gradient, as on the device.
    -> (final parameters as numpy arrays of `dtype`, [(L_cls, L_box)] per step)"""
    import torch
    dtype = dtype or torch.float64
    nt = n_towers_of(P)
    Pt = {n: torch.as_tensor(np.asarray(P[n])).to(dtype).clone().requires_grad_(True) for n in names(nt)}
    opt = torch.optim.SGD([{"params": [Pt[n] for n in Pt if is_weight(n)], "weight_decay": weight_decay},
                           {"params": [Pt[n] for n in Pt if not is_weight(n)], "weight_decay": 0.0}], lr=lr, momentum=momentum)
    losses = []
    for xs, rois, gt, labels, k, drop in batches:
        xs = [torch.as_tensor(np.asarray(x)).to(dtype) for x in xs]
        r, g = torch.as_tensor(np.asarray(rois)).to(dtype), torch.as_tensor(np.asarray(gt)).to(dtype)
        y = torch.as_tensor(np.asarray(labels)).long()
        B = xs[0].shape[0]
        y7s = []
        for t in range(nt):
            m = torch.einsum("bkp,nk->bnp", xs[t], Pt["t%d.mix_w" % t]) + Pt["t%d.mix_b" % t][None, :, None]
            y6 = torch.relu(m.reshape(B, -1) @ Pt["t%d.fc6_w" % t].t() + Pt["t%d.fc6_b" % t])
            if drop is not None:
                y6 = y6 * torch.as_tensor(np.asarray(drop[t][0])).to(dtype)
            y7 = torch.relu(y6 @ Pt["t%d.fc7_w" % t].t() + Pt["t%d.fc7_b" % t])
            if drop is not None:
                y7 = y7 * torch.as_tensor(np.asarray(drop[t][1])).to(dtype)
            y7s.append(y7)
        F = y7s[0].shape[1]
        cat = torch.cat(y7s, 1)
        z = cat[:, :(nt - 1) * F] @ Pt["cls_w"].t() + Pt["cls_b"]
        that = cat[:, (nt - 1) * F:] @ Pt["bbox_w"].t() + Pt["bbox_b"]
        C = that.shape[1] // 4
        L_cls = torch.nn.CrossEntropyLoss()(z[:, k * C:(k + 1) * C], y)
        fg = torch.nonzero(y > 0)[:, 0]
        L_box = that.sum() * 0.0
        if fg.numel():
            rf, gf = r[fg], g[fg]
            xc, yc, w, h = (rf[:, 0] + rf[:, 2]) * 0.5, (rf[:, 1] + rf[:, 3]) * 0.5, rf[:, 2] - rf[:, 0], rf[:, 3] - rf[:, 1]
            xtc, ytc, wt, ht = (gf[:, 0] + gf[:, 2]) * 0.5, (gf[:, 1] + gf[:, 3]) * 0.5, gf[:, 2] - gf[:, 0], gf[:, 3] - gf[:, 1]
            t = torch.stack([(xtc - xc) / w, (ytc - yc) / h, torch.log(wt / w), torch.log(ht / h)], 1)
            if std is not None and std[0] != 0:
                t = (t - torch.tensor(list(mean), dtype=dtype)) / torch.tensor(list(std), dtype=dtype)
            cols = 4 * y[fg][:, None] + torch.arange(4)[None, :]
            L_box = bbox_weight * torch.nn.SmoothL1Loss(reduction="sum")(that[fg[:, None], cols], t) / B
        opt.zero_grad()
        (L_cls + L_box).backward()
        for p_ in Pt.values():      # a tensor the loss does not reach (a classifier not selected) still takes its step
            if p_.grad is None:
                p_.grad = torch.zeros_like(p_)
        opt.step()
        losses.append((float(L_cls.detach()), float(L_box.detach())))
    return {n: Pt[n].detach().numpy() for n in Pt}, losses


def make_batch(seed, n, C, n_bg, H, W):
    """one image's rows (tests/test_gpu_train.py's rule): the first n_bg background; of the foreground rows every third regresses to a GT
    box half a box width away (normalised |d| >= 1, the linear branch), the others to one within a pixel (|d| < 1, the quadratic branch)"""
    rng = np.random.default_rng(seed)
    im = rng.random((3, H, W), dtype=np.float32)
    c = rng.uniform([24, 24], [W - 24, H - 24], (n, 2))
    wh = rng.uniform(12, 44, (n, 2))
    rois = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    gt = rois + rng.normal(0, 0.4, (n, 4)).astype(np.float32)
    far = np.arange(n) % 3 == 0
    wv = (rois[:, 2] - rois[:, 0])[:, None]
    gt[far] = rois[far] + 0.5 * wv[far] * np.array([1, 0, 1, 0], np.float32)
    labels = rng.integers(1, C, n).astype(np.int32)
    labels[:n_bg] = 0
    gt[:n_bg] = 0
    return im, rois.astype(np.float32), gt.astype(np.float32), labels
