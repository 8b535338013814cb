"""Dropout behind fc6 and fc7 restated for the tests (test infrastructure; include/mpn.h mpn_frcnn_train_set_dropout, DESIGN.md section
13.6): Philox4x32-10 and the keep mask as a pure function of (seed, step, layer, row, column) in numpy, one training step of the head
in float64 with the masks applied (tests/train_np.py's loss and optim.sgd), and the same step by PyTorch-CPU autograd in a chosen dtype
with the mask as a constant multiplier — in float64 it checks this file (tests/test_dropout_cpu.py), in float32 it is the yardstick the
device is judged against (tests/test_gpu_train_dropout.py)."""
import numpy as np

import train_np as T

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (broadcast against each other) of 32-bit values -> [..., 4] uint32.  One round:
    (hi0, lo0) = M0 * c0, (hi1, lo1) = M1 * c2, c = (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key is bumped between rounds."""
    c = np.asarray(counter, np.uint64)
    k = np.asarray(key, np.uint64)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    m32 = np.uint64(MASK32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2     # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(W0)) & m32, (k1 + np.uint64(W1)) & m32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(np.uint32)


def threshold(rate):
    """T = floor(rate * 2^32) in double, rate being the float the C ABI takes"""
    return int(np.floor(float(np.float32(rate)) * 4294967296.0))


def scale(rate):
    """s = 1.0f / (1.0f - rate) in fp32"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(rate))


def words(seed, step, layer, B, N):
    """[B, N] uint32: the word of every element — word col & 3 of Philox(counter = (row, col >> 2, layer, step & 0xffffffff),
    key = (seed & 0xffffffff, seed >> 32)), the seed taken as 64 bits"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    G = (N + 3) // 4
    ctr = np.zeros((B, G, 4), np.uint64)
    ctr[..., 0] = np.arange(B, dtype=np.uint64)[:, None]
    ctr[..., 1] = np.arange(G, dtype=np.uint64)[None, :]
    ctr[..., 2] = layer
    ctr[..., 3] = int(step) & MASK32
    out = philox4x32_10(ctr, np.array([seed & MASK32, seed >> 32], np.uint64))
    return out.reshape(B, G * 4)[:, :N]


def keep_mask(seed, step, layer, B, N, rate):
    """[B, N] bool: an element is kept iff its word >= T"""
    return words(seed, step, layer, B, N) >= np.uint32(threshold(rate))


def multipliers(seed, step, B, F, rate):
    """(m6, m7) [B, F] float32: s where kept, 0 where dropped — what y6 / y7 are multiplied with"""
    s = scale(rate)
    return tuple(np.where(keep_mask(seed, step, layer, B, F, rate), s, np.float32(0)).astype(np.float32) for layer in (0, 1))


def loss_and_grads(P, x, rois, gt, labels, m6, m7, mean, std, bbox_weight=1.0, depth=2):
    """train_np.loss_and_grads with y6 = relu(.) * m6 and y7 = relu(.) * m7 (nn.Dropout v2 in training mode), float64"""
    P = {k: np.asarray(P[k], np.float64) for k in T.TENSORS}
    x, m6, m7 = np.asarray(x, np.float64), np.asarray(m6, np.float64), np.asarray(m7, np.float64)
    labels = np.asarray(labels, np.int64)
    B = x.shape[0]
    a6 = x @ P["fc6_w"].T + P["fc6_b"]
    y6 = np.maximum(a6, 0.0) * m6
    a7 = y6 @ P["fc7_w"].T + P["fc7_b"]
    y7 = np.maximum(a7, 0.0) * m7
    z, that = y7 @ P["cls_w"].T + P["cls_b"], y7 @ P["bbox_w"].T + P["bbox_b"]
    mx = z.max(1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(z - mx).sum(1))
    L_cls = float((lse - z[np.arange(B), labels]).sum() / B)
    gz = np.exp(z - lse[:, None])
    gz[np.arange(B), labels] -= 1.0
    gz /= B
    t, fg = T.targets(rois, gt, labels, mean, std)
    gt_hat = np.zeros_like(that)
    idx = np.nonzero(fg)[0]
    cols = 4 * labels[idx][:, None] + np.arange(4)[None, :]
    d = that[idx[:, None], cols] - t[idx]
    L_box = float(bbox_weight * np.where(np.abs(d) < 1.0, 0.5 * d * d, np.abs(d) - 0.5).sum() / B)
    gt_hat[idx[:, None], cols] = bbox_weight / B * np.clip(d, -1.0, 1.0)
    G = {"cls_w": gz.T @ y7, "cls_b": gz.sum(0), "bbox_w": gt_hat.T @ y7, "bbox_b": gt_hat.sum(0)}
    if depth >= 1:
        g7 = (gz @ P["cls_w"] + gt_hat @ P["bbox_w"]) * m7 * (a7 > 0)
        G["fc7_w"], G["fc7_b"] = g7.T @ y6, g7.sum(0)
        if depth >= 2:
            g6 = (g7 @ P["fc7_w"]) * m6 * (a6 > 0)
            G["fc6_w"], G["fc6_b"] = g6.T @ x, g6.sum(0)
    return (L_cls, L_box), G, d


class Sgd64(T.Sgd64):
    """train_np.Sgd64 whose step takes the two multiplier matrices"""

    def step(self, x, rois, gt, labels, m6, m7, lr):
        loss, G, d = loss_and_grads(self.P, x, rois, gt, labels, m6, m7, self.mean, self.std, self.bbox_weight, self.depth)
        for k in T.TRAINED[self.depth]:
            g = G[k] + (self.wd * self.P[k] if k in T.WEIGHTS else 0.0)
            self.V[k] = self.momentum * self.V[k] + g
            self.P[k] = self.P[k] - lr * self.V[k]
        return loss, d


def torch_steps(P, batches, lr, depth=2, momentum=0.9, weight_decay=5e-4, bbox_weight=1.0, mean=None, std=None, dtype=None):
    """train_np.torch_steps with dropout: batches [(x, rois, gt, labels, m6, m7)], the multipliers constants of the graph.
    lr: one rate, or one per batch.  -> (final parameters as numpy arrays of `dtype`, [(L_cls, L_box)] per step)"""
    import torch
    dtype = dtype or torch.float64
    Pt = {k: torch.as_tensor(np.asarray(P[k])).to(dtype).clone() for k in T.TENSORS}
    for k in T.TRAINED[depth]:
        Pt[k].requires_grad_(True)
    lrs = list(lr) if isinstance(lr, (list, tuple)) else [lr] * len(batches)
    lr = lrs[0]
    opt = torch.optim.SGD([{"params": [Pt[k] for k in T.TRAINED[depth] if k in T.WEIGHTS], "weight_decay": weight_decay},
                           {"params": [Pt[k] for k in T.TRAINED[depth] if k in T.BIASES], "weight_decay": 0.0}], lr=lr, momentum=momentum)
    losses = []
    for (x, rois, gt, labels, m6, m7), lr_i in zip(batches, lrs):
        for grp in opt.param_groups:
            grp["lr"] = lr_i
        x = torch.as_tensor(np.asarray(x)).to(dtype)
        m6, m7 = torch.as_tensor(np.asarray(m6)).to(dtype), torch.as_tensor(np.asarray(m7)).to(dtype)
        r, g = torch.as_tensor(np.asarray(rois)).to(dtype), torch.as_tensor(np.asarray(gt)).to(dtype)
        y = torch.as_tensor(np.asarray(labels)).long()
        B = x.shape[0]
        y6 = torch.relu(x @ Pt["fc6_w"].t() + Pt["fc6_b"]) * m6
        y7 = torch.relu(y6 @ Pt["fc7_w"].t() + Pt["fc7_b"]) * m7
        z, that = y7 @ Pt["cls_w"].t() + Pt["cls_b"], y7 @ Pt["bbox_w"].t() + Pt["bbox_b"]
        L_cls = torch.nn.CrossEntropyLoss()(z, y)
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
        opt.step()
        losses.append((float(L_cls.detach()), float(L_box.detach())))
    return {k: Pt[k].detach().numpy() for k in T.TENSORS}, losses
