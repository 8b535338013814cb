"""Float64 restatement of one training step of the Fast R-CNN head (test infrastructure): the loss of train.lua:154-158 with
BBoxRegressionCriterion.lua's smooth L1, the targets of BatchProviderROI.lua:125-131 / utils.lua:171-184, the backward pass of the three
Linear layers behind the ROI pooling and optim.sgd as engines/Optim.lua drives it (dampening 0, no Nesterov, biases never decay).
Everything starts from the pooled operand x [B, K6] (Torch order: channel-major, then bin), so the frozen trunk is no part of it.

torch_steps is the same computation by PyTorch-CPU autograd + torch.optim.SGD in a chosen dtype: in float64 it checks this file
(tests/test_train_cpu.py), in float32 it is the yardstick the device is judged against (tests/test_gpu_train.py).
setup_one_np / select_np restate the ROI sampler's rules (BatchProviderROI.lua:39-49, BatchProviderBase.lua:77-107) with plain loops."""
import numpy as np

WEIGHTS = ("fc6_w", "fc7_w", "cls_w", "bbox_w")
BIASES = ("fc6_b", "fc7_b", "cls_b", "bbox_b")
TENSORS = ("fc6_w", "fc6_b", "fc7_w", "fc7_b", "cls_w", "cls_b", "bbox_w", "bbox_b")
TRAINED = {0: ("cls_w", "cls_b", "bbox_w", "bbox_b"), 1: ("fc7_w", "fc7_b", "cls_w", "cls_b", "bbox_w", "bbox_b"), 2: TENSORS}


def convert_to(rois, gt):
    """utils.convertTo (utils.lua:171-184), float64"""
    r, t = np.asarray(rois, np.float64), np.asarray(gt, np.float64)
    xc, yc, w, h = (r[:, 0] + r[:, 2]) * 0.5, (r[:, 1] + r[:, 3]) * 0.5, r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
    xtc, ytc, wt, ht = (t[:, 0] + t[:, 2]) * 0.5, (t[:, 1] + t[:, 3]) * 0.5, t[:, 2] - t[:, 0], t[:, 3] - t[:, 1]
    return np.stack([(xtc - xc) / w, (ytc - yc) / h, np.log(wt / w), np.log(ht / h)], 1)


def targets(rois, gt, labels, mean, std):
    """[B,4] normalised regression targets (rows with label 0: zeros, never read) and the foreground mask"""
    fg = np.asarray(labels) > 0
    t = np.zeros((len(labels), 4))
    if fg.any():
        t[fg] = convert_to(np.asarray(rois)[fg], np.asarray(gt)[fg])
        if std is not None and std[0] != 0:
            t[fg] = (t[fg] - np.asarray(mean, np.float64)) / np.asarray(std, np.float64)
    return t, fg


def forward(P, x):
    y6 = np.maximum(x @ P["fc6_w"].T + P["fc6_b"], 0.0)
    y7 = np.maximum(y6 @ P["fc7_w"].T + P["fc7_b"], 0.0)
    return y6, y7, y7 @ P["cls_w"].T + P["cls_b"], y7 @ P["bbox_w"].T + P["bbox_b"]


def loss_and_grads(P, x, rois, gt, labels, mean, std, bbox_weight=1.0, depth=2):
    """-> ((L_cls, L_box), {tensor: gradient} for the tensors `depth` trains, d) with d [n_fg, 4] the smooth-L1 arguments"""
    P = {k: np.asarray(P[k], np.float64) for k in TENSORS}
    x = np.asarray(x, np.float64)
    labels = np.asarray(labels, np.int64)
    B, C = x.shape[0], P["cls_w"].shape[0]
    y6, y7, z, that = forward(P, x)
    mx = z.max(1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(z - mx).sum(1))
    L_cls = float((lse - z[np.arange(B), labels]).sum() / B)
    soft = np.exp(z - lse[:, None])
    gz = soft.copy()
    gz[np.arange(B), labels] -= 1.0
    gz /= B
    t, fg = targets(rois, gt, labels, mean, std)
    gt_hat = np.zeros_like(that)
    idx = np.nonzero(fg)[0]
    cols = 4 * labels[idx][:, None] + np.arange(4)[None, :]
    d = that[idx[:, None], cols] - t[idx]
    sl1 = np.where(np.abs(d) < 1.0, 0.5 * d * d, np.abs(d) - 0.5)
    L_box = float(bbox_weight * sl1.sum() / B)
    gt_hat[idx[:, None], cols] = bbox_weight / B * np.clip(d, -1.0, 1.0)
    G = {"cls_w": gz.T @ y7, "cls_b": gz.sum(0), "bbox_w": gt_hat.T @ y7, "bbox_b": gt_hat.sum(0)}
    if depth >= 1:
        g7 = (gz @ P["cls_w"] + gt_hat @ P["bbox_w"]) * (y7 > 0)
        G["fc7_w"], G["fc7_b"] = g7.T @ y6, g7.sum(0)
        if depth >= 2:
            g6 = (g7 @ P["fc7_w"]) * (y6 > 0)
            G["fc6_w"], G["fc6_b"] = g6.T @ x, g6.sum(0)
    return (L_cls, L_box), G, d


class Sgd64(object):
    """optim.sgd over the head's tensors in float64: g += wd * w for weights only, v = momentum * v + g, w -= lr * v"""

    def __init__(self, P, depth=2, momentum=0.9, weight_decay=5e-4, bbox_weight=1.0, mean=None, std=None):
        self.P = {k: np.array(np.asarray(P[k]), np.float64) for k in TENSORS}
        self.V = {k: np.zeros_like(self.P[k]) for k in TRAINED[depth]}
        self.depth, self.momentum, self.wd, self.bbox_weight, self.mean, self.std = depth, momentum, weight_decay, bbox_weight, mean, std

    def step(self, x, rois, gt, labels, lr):
        loss, G, d = loss_and_grads(self.P, x, rois, gt, labels, self.mean, self.std, self.bbox_weight, self.depth)
        for k in TRAINED[self.depth]:
            g = G[k] + (self.wd * self.P[k] if k in WEIGHTS else 0.0)
            self.V[k] = self.momentum * self.V[k] + g
            self.P[k] = self.P[k] - lr * self.V[k]
        return loss, d


def torch_steps(P, batches, lr, depth=2, momentum=0.9, weight_decay=5e-4, bbox_weight=1.0, mean=None, std=None, dtype=None):
    """The same steps by PyTorch-CPU: CrossEntropyLoss + masked SmoothL1Loss(reduction='sum') / B, autograd, torch.optim.SGD with the
    biases in a weight_decay = 0 group.  batches: [(x [B,K6], rois, gt, labels)].  Everything — targets included — in `dtype`.
    -> (final parameters as numpy arrays of that dtype, [(L_cls, L_box)] per step)"""
    import torch
    dtype = dtype or torch.float64
    T = {k: torch.as_tensor(np.asarray(P[k])).to(dtype).clone() for k in TENSORS}
    for k in TRAINED[depth]:
        T[k].requires_grad_(True)
    opt = torch.optim.SGD([{"params": [T[k] for k in TRAINED[depth] if k in WEIGHTS], "weight_decay": weight_decay},
                           {"params": [T[k] for k in TRAINED[depth] if k in BIASES], "weight_decay": 0.0}], lr=lr, momentum=momentum)
    losses = []
    for x, rois, gt, labels in batches:
        x = torch.as_tensor(np.asarray(x)).to(dtype)
        r, g = torch.as_tensor(np.asarray(rois)).to(dtype), torch.as_tensor(np.asarray(gt)).to(dtype)
        y = torch.as_tensor(np.asarray(labels)).long()
        B = x.shape[0]
        y6 = torch.relu(x @ T["fc6_w"].t() + T["fc6_b"])
        y7 = torch.relu(y6 @ T["fc7_w"].t() + T["fc7_b"])
        z, that = y7 @ T["cls_w"].t() + T["cls_b"], y7 @ T["bbox_w"].t() + T["bbox_b"]
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
    return {k: T[k].detach().numpy() for k in TENSORS}, losses


def setup_one_np(overlap, fg_threshold=0.5, bg_threshold=(0.1, 0.5)):
    """BatchProviderROI:setupOne's two index sets with plain loops: fg = overlap >= fg_threshold, bg = lo <= overlap < hi"""
    fg, bg = [], []
    for i, o in enumerate(overlap):
        if o >= np.float32(fg_threshold):
            fg.append(i)
        if o >= np.float32(bg_threshold[0]) and o < np.float32(bg_threshold[1]):
            bg.append(i)
    return bg, fg


def select_counts_np(n_bg, n_fg, batch_size=128, fg_fraction=0.25):
    """rows selectBBoxesOne draws: (min(bg_num, n_bg), min(fg_num, n_fg)) with fg_num = fg_fraction * batch_size, bg_num the rest"""
    fg_num = int(fg_fraction * batch_size)
    return min(batch_size - fg_num, n_bg), min(fg_num, n_fg)
