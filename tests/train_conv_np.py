"""Float64 / float32 restatement of one training step at depth MPN_TRAIN_CONV(k) (test infrastructure): the head
stage of tests/train_np.py from the pooled operand, extended to hand back the gradient at the pooled features, and the BLOCK stage — the
conv layers above the trunk's last pooling layer rebuilt from their saved input map, the ROI pooling as a gather at a GIVEN argmax, the
ReLUs as GIVEN masks — by PyTorch-CPU autograd in a chosen dtype, then optim.sgd (torch.optim.SGD, biases in a weight_decay = 0 group).

With the device's masks and argmax handed in, the float side never decides where a ReLU is open or which cell a bin picked, so no case
is ever ambiguous; with its own (masks = None, argmax = None) it is plain autograd through relu and a max over each bin's window
(tests/test_train_conv_cpu.py checks the two against each other).  In float64 it is the reference, in float32 the yardstick."""
import numpy as np
import torch

import train_np as T

U = 2.0 ** -24


def roi_windows(rois5, H, W, PH, PW, scale):
    """bin windows of inn.ROIPooling's CUDA branch (coordinate offset 1, fp32 arithmetic as roi_bin_bounds): [n][bin] -> (hs, he, ws, we)"""
    f = np.float32
    rnd = lambda v: int(np.floor(abs(float(v)) + 0.5)) * (1 if v >= 0 else -1)   # roundf: halves away from zero
    out = []
    for r in np.asarray(rois5, np.float32):
        sw, sh = rnd(f(f(r[1] - f(1)) * f(scale))), rnd(f(f(r[2] - f(1)) * f(scale)))
        ew, eh = rnd(f(f(r[3] - f(1)) * f(scale))), rnd(f(f(r[4] - f(1)) * f(scale)))
        rw, rh = max(ew - sw + 1, 1), max(eh - sh + 1, 1)
        bh, bw = f(rh) / f(PH), f(rw) / f(PW)
        row = []
        for ph in range(PH):
            for pw in range(PW):
                hs, he = int(np.floor(f(ph) * bh)) + sh, int(np.ceil(f(ph + 1) * bh)) + sh
                ws, we = int(np.floor(f(pw) * bw)) + sw, int(np.ceil(f(pw + 1) * bw)) + sw
                row.append((min(max(hs, 0), H), min(max(he, 0), H), min(max(ws, 0), W), min(max(we, 0), W)))
        out.append(row)
    return out


def own_argmax(amap, rois5, PH, PW, scale):
    """[n, C, PH*PW] int64: first strict maximum of each bin's window in row-major scan, -1 for an empty bin (amap [C,h,w], any dtype)"""
    a = np.asarray(amap)
    C, H, W = a.shape
    win = roi_windows(rois5, H, W, PH, PW, scale)
    out = -np.ones((len(win), C, PH * PW), np.int64)
    for n, row in enumerate(win):
        for b, (hs, he, ws, we) in enumerate(row):
            if he <= hs or we <= ws:
                continue
            sub = a[:, hs:he, ws:we].reshape(C, -1)
            k = sub.argmax(1)   # numpy: the first maximum
            out[n, :, b] = (hs + k // (we - ws)) * W + ws + k % (we - ws)
    return out


def gather_pool(amap, argmax):
    """amap [C,h,w] tensor, argmax [n,C,PP] (-1: empty) -> pooled [n, C, PP]"""
    C = amap.shape[0]
    idx = torch.as_tensor(np.asarray(argmax), dtype=torch.long)
    flat = amap.reshape(C, -1)
    g = torch.gather(flat.unsqueeze(0).expand(idx.shape[0], C, flat.shape[1]), 2, idx.clamp(min=0))
    return torch.where(idx >= 0, g, torch.zeros((), dtype=amap.dtype))


class Trainer(object):
    """The head's eight tensors + the block's conv layers, trained by autograd + torch.optim.SGD in `dtype`.
    P: numpy dict with T.TENSORS; conv: [(w [Cout,Cin,3,3], b [Cout])] of the K block layers, first to last; depth = 2 + k."""

    def __init__(self, P, conv, depth, momentum, weight_decay, bbox_weight=1.0, mean=None, std=None, dtype=torch.float64, lr=1.0):
        self.dtype, self.k, self.K = dtype, depth - 2, len(conv)
        self.bbox_weight, self.mean, self.std = bbox_weight, mean, std
        self.T = {k: torch.as_tensor(np.asarray(P[k])).to(dtype).clone() for k in T.TENSORS}
        self.cw = [torch.as_tensor(np.asarray(w)).to(dtype).clone() for w, _ in conv]
        self.cb = [torch.as_tensor(np.asarray(b)).to(dtype).clone() for _, b in conv]
        ws = [self.T[k] for k in T.WEIGHTS] + self.cw[self.K - self.k:]
        bs = [self.T[k] for k in T.BIASES] + self.cb[self.K - self.k:]
        for t in ws + bs:
            t.requires_grad_(True)
        self.opt = torch.optim.SGD([{"params": ws, "weight_decay": weight_decay}, {"params": bs, "weight_decay": 0.0}], lr=lr, momentum=momentum)

    def head(self, x, rois, gt, labels):
        """train_np.torch_steps' forward and loss on the leaf x -> (L_cls, L_box) tensors"""
        dtype, Tn = self.dtype, self.T
        r, g = torch.as_tensor(np.asarray(rois)).to(dtype), torch.as_tensor(np.asarray(gt)).to(dtype)
        y = torch.as_tensor(np.asarray(labels)).long()
        B = x.shape[0]
        y6 = torch.relu(x @ Tn["fc6_w"].t() + Tn["fc6_b"])
        y7 = torch.relu(y6 @ Tn["fc7_w"].t() + Tn["fc7_b"])
        z, that = y7 @ Tn["cls_w"].t() + Tn["cls_b"], y7 @ Tn["bbox_w"].t() + Tn["bbox_b"]
        L_cls = torch.nn.CrossEntropyLoss()(z, y)
        fg = torch.nonzero(y > 0)[:, 0]
        L_box = that.sum() * 0.0
        if fg.numel():
            rf, gf = r[fg], g[fg]
            xc, yc, w, h = (rf[:, 0] + rf[:, 2]) * 0.5, (rf[:, 1] + rf[:, 3]) * 0.5, rf[:, 2] - rf[:, 0], rf[:, 3] - rf[:, 1]
            xtc, ytc, wt, ht = (gf[:, 0] + gf[:, 2]) * 0.5, (gf[:, 1] + gf[:, 3]) * 0.5, gf[:, 2] - gf[:, 0], gf[:, 3] - gf[:, 1]
            t = torch.stack([(xtc - xc) / w, (ytc - yc) / h, torch.log(wt / w), torch.log(ht / h)], 1)
            if self.std is not None and self.std[0] != 0:
                t = (t - torch.tensor(list(self.mean), dtype=dtype)) / torch.tensor(list(self.std), dtype=dtype)
            cols = 4 * y[fg][:, None] + torch.arange(4)[None, :]
            L_box = self.bbox_weight * torch.nn.SmoothL1Loss(reduction="sum")(that[fg[:, None], cols], t) / B
        return L_cls, L_box

    def block(self, a0, masks=None):
        """the k TRAINED layers on the saved input map a0 [Cin,h,w] of the first of them: conv2d + the GIVEN masks (masks[j]: bool [C,h,w]
        of the j-th trained layer's output) or, without masks, relu -> the last layer's output [C,h,w]"""
        a = torch.as_tensor(np.asarray(a0)).to(self.dtype)[None]
        for j in range(self.k):
            l = self.K - self.k + j
            a = torch.nn.functional.conv2d(a, self.cw[l], self.cb[l], padding=1)
            a = torch.relu(a) if masks is None else a * torch.as_tensor(np.asarray(masks[j])).to(self.dtype)[None]
        return a[0]

    def step(self, x, rois, gt, labels, images, lr, PH=7, PW=7, scale=0.25):
        """one step.  x [B,K6] the pooled operand the head starts from; images: [(a0, masks or None, argmax [n,C,PP] or None, rois5 [n,5])]
        in train_add order, rows in the same order as x's.  -> ((L_cls, L_box), dx6 [B,K6] before the [x > 0] mask)"""
        for gr in self.opt.param_groups:
            gr["lr"] = lr
        self.opt.zero_grad()
        xt = torch.as_tensor(np.asarray(x)).to(self.dtype).clone().requires_grad_(True)
        L_cls, L_box = self.head(xt, rois, gt, labels)
        (L_cls + L_box).backward()
        dx6 = xt.grad.detach()
        row = 0
        for a0, masks, argmax, rois5 in images:
            n = len(rois5)
            if self.k > 0:
                top = self.block(a0, masks)
                am = own_argmax(top.detach().numpy(), rois5, PH, PW, scale) if argmax is None else argmax
                pooled = gather_pool(top, am)
                pooled.backward(dx6[row:row + n].reshape(pooled.shape))
            row += n
        self.opt.step()
        return (float(L_cls.detach()), float(L_box.detach())), dx6.numpy()

    def params(self):
        out = {k: self.T[k].detach().numpy() for k in T.TENSORS}
        out["conv_w"] = [w.detach().numpy() for w in self.cw]
        out["conv_b"] = [b.detach().numpy() for b in self.cb]
        return out


def roi_pool_backward_np(grad_out, argmax, rois5, B, C, H, W, dtype=np.float32):
    """the contract's ordered sum with plain loops: per cell, rows of its map ascending, bins ascending; adds in `dtype` from +0.0"""
    g, am = np.asarray(grad_out).reshape(len(rois5), C, -1), np.asarray(argmax).reshape(len(rois5), C, -1)
    out = np.zeros((B, C, H * W), dtype)
    for n in range(len(rois5)):   # rows ascending; inside a row bins ascending: each cell's sum sees its terms in the contract's order
        b = min(max(int(rois5[n][0]) - 1, 0), B - 1)
        for c in range(C):
            for k in range(g.shape[2]):
                i = am[n, c, k]
                if i >= 0:
                    out[b, c, i] = dtype(out[b, c, i] + dtype(g[n, c, k]))
    return out.reshape(B, C, H, W)
