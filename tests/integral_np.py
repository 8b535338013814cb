"""Float64 restatement of one training step of a Fast R-CNN head that holds the integral loss's K classifiers (test infrastructure;
model_utils.lua:275-317, train.lua:288-294).  It extends tests/train_np.py: P["cls_w"] is [K*C, F] and
P["cls_b"] [K*C], the K classifiers stacked in head order; a step's loss reads classifier k alone, so the selected classifier, bbox,
fc7 and fc6 get train_np's gradients of the head [cls_k | bbox] and every other classifier's gradient is exactly zero.  optim.sgd
still steps ALL of them (engines/Optim.lua updates every module on every call): weight decay and momentum act on the unselected ones.

torch_steps is the same by PyTorch-CPU autograd + torch.optim.SGD with the stacked classifier as ONE leaf: autograd hands the
unselected rows a zero gradient, and torch.optim.SGD decays and steps them as optim.sgd does."""
import numpy as np

import train_np as T

TENSORS, TRAINED, WEIGHTS, BIASES = T.TENSORS, T.TRAINED, T.WEIGHTS, T.BIASES


def head_rows(K, k, C):
    """rows of the stacked classifier that belong to head k"""
    assert 0 <= k < K
    return slice(k * C, (k + 1) * C)


def loss_and_grads(P, x, rois, gt, labels, mean, std, K, k, bbox_weight=1.0, depth=2):
    """train_np.loss_and_grads on the head [cls_k | bbox]; G["cls_w"] / G["cls_b"] come back in the stacked shape, zero outside head k"""
    P = {n: np.asarray(P[n], np.float64) for n in TENSORS}
    assert P["cls_w"].shape[0] % K == 0
    C = P["cls_w"].shape[0] // K
    rows = head_rows(K, k, C)
    Pk = dict(P)
    Pk["cls_w"], Pk["cls_b"] = P["cls_w"][rows], P["cls_b"][rows]
    loss, Gk, d = T.loss_and_grads(Pk, x, rois, gt, labels, mean, std, bbox_weight, depth)
    G = dict(Gk)
    G["cls_w"], G["cls_b"] = np.zeros_like(P["cls_w"]), np.zeros_like(P["cls_b"])
    G["cls_w"][rows], G["cls_b"][rows] = Gk["cls_w"], Gk["cls_b"]
    return loss, G, d


class Sgd64(object):
    """optim.sgd over the K-head's tensors in float64; step(..., k) trains classifier k, and steps every tensor the depth trains"""

    def __init__(self, P, K, depth=2, momentum=0.9, weight_decay=5e-4, bbox_weight=1.0, mean=None, std=None):
        self.K = int(K)
        self.P = {n: np.array(np.asarray(P[n]), np.float64) for n in TENSORS}
        self.V = {n: np.zeros_like(self.P[n]) for n in TRAINED[depth]}
        self.depth, self.momentum, self.wd, self.bbox_weight, self.mean, self.std = depth, momentum, weight_decay, bbox_weight, mean, std

    def step(self, x, rois, gt, labels, lr, k):
        loss, G, d = loss_and_grads(self.P, x, rois, gt, labels, self.mean, self.std, self.K, k, self.bbox_weight, self.depth)
        for n in TRAINED[self.depth]:
            g = G[n] + (self.wd * self.P[n] if n in WEIGHTS else 0.0)
            self.V[n] = self.momentum * self.V[n] + g
            self.P[n] = self.P[n] - lr * self.V[n]
        return loss, d


def torch_steps(P, batches, heads, lr, K, depth=2, momentum=0.9, weight_decay=5e-4, bbox_weight=1.0, mean=None, std=None, dtype=None):
    """train_np.torch_steps with the stacked classifier: batches [(x, rois, gt, labels)], heads [k] per batch.
    -> (final parameters as numpy arrays of `dtype`, [(L_cls, L_box)] per step)"""
    import torch
    dtype = dtype or torch.float64
    Tn = {n: torch.as_tensor(np.asarray(P[n])).to(dtype).clone() for n in TENSORS}
    C = Tn["cls_w"].shape[0] // K
    for n in TRAINED[depth]:
        Tn[n].requires_grad_(True)
    opt = torch.optim.SGD([{"params": [Tn[n] for n in TRAINED[depth] if n in WEIGHTS], "weight_decay": weight_decay},
                           {"params": [Tn[n] for n in TRAINED[depth] if n in BIASES], "weight_decay": 0.0}], lr=lr, momentum=momentum)
    losses = []
    for (x, rois, gt, labels), k in zip(batches, heads):
        x = torch.as_tensor(np.asarray(x)).to(dtype)
        r, g = torch.as_tensor(np.asarray(rois)).to(dtype), torch.as_tensor(np.asarray(gt)).to(dtype)
        y = torch.as_tensor(np.asarray(labels)).long()
        B = x.shape[0]
        y6 = torch.relu(x @ Tn["fc6_w"].t() + Tn["fc6_b"])
        y7 = torch.relu(y6 @ Tn["fc7_w"].t() + Tn["fc7_b"])
        zk, that = y7 @ Tn["cls_w"].t() + Tn["cls_b"], y7 @ Tn["bbox_w"].t() + Tn["bbox_b"]
        z = zk[:, k * C:(k + 1) * C]   # the selector: the loss reads classifier k (the others get a zero, not a missing, gradient)
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
            pred = that[fg[:, None], cols]
            L_box = bbox_weight * torch.nn.SmoothL1Loss(reduction="sum")(pred, t) / B
        opt.zero_grad()
        (L_cls + L_box).backward()
        opt.step()
        losses.append((float(L_cls.detach()), float(L_box.detach())))
    return {n: Tn[n].detach().numpy() for n in TENSORS}, losses
