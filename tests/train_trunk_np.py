"""Float64 / float32 restatement of one training step at depth MPN_TRAIN_TRUNK(k) (test infrastructure):
tests/train_conv_np.py's Trainer with nn.SpatialMaxPooling(2,2,2,2):ceil() layers among the trained conv layers.  The pool is a gather at
a ROUTING — per window the flat index (y * W + x) of the cell its value comes from — so that, as with the ReLU masks and the ROI pooling's
argmax, the float side can be handed the device's decisions and never decides anything itself; without a routing it takes its own by the
first-maximum rule (first_max_route: the forward's scan from -inf with v > m over (2Y,2X), (2Y,2X+1), (2Y+1,2X), (2Y+1,2X+1), cells outside
the map skipped).  tests/test_train_trunk_cpu.py checks the whole against plain autograd (conv2d / relu / max_pool2d(ceil_mode=True)).

maxpool_backward_np is the contract of mpn_maxpool2x2_ceil_backward written with plain numpy, cell by cell of the window."""
import numpy as np
import torch

import train_conv_np as TC


def _window_cells(H, W):
    """the four cells of every window in the forward's scan order: [(ys [Ho], xs [Wo], inside [Ho, Wo])]"""
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    out = []
    for dy in (0, 1):
        for dx in (0, 1):
            ys, xs = 2 * np.arange(Ho) + dy, 2 * np.arange(Wo) + dx
            inside = (ys < H)[:, None] & (xs < W)[None, :]
            out.append((np.minimum(ys, H - 1), np.minimum(xs, W - 1), inside))
    return out


def first_max_route(x):
    """x [C,H,W] -> route [C,Ho,Wo] int64: y * W + x of the cell the forward's scan ends on (the first maximum in row-major order),
    -1 for a window that holds only NaN"""
    x = np.asarray(x)
    C, H, W = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    m = np.full((C, Ho, Wo), -np.inf, x.dtype)
    route = -np.ones((C, Ho, Wo), np.int64)
    for ys, xs, inside in _window_cells(H, W):
        v = x[:, ys][:, :, xs]
        take = inside[None] & (v > m)
        m = np.where(take, v, m)
        route = np.where(take, (ys[:, None] * W + xs[None, :])[None], route)
    return route


def maxpool_backward_np(x, gy, relu_mask):
    """dX of the contract: gy's value on the cell the scan ends on (relu_mask: only where that cell is > 0), +0.0 on every other cell"""
    x, gy = np.asarray(x), np.asarray(gy)
    C, H, W = x.shape
    dx = np.zeros((C, H * W), gy.dtype)
    route = first_max_route(x)
    flat = x.reshape(C, -1)
    for c in range(C):
        r, g = route[c].reshape(-1), gy[c].reshape(-1)
        ok = r >= 0
        if relu_mask:
            ok = ok & (flat[c][np.maximum(r, 0)] > 0)
        dx[c, r[ok]] = g[ok]   # windows do not overlap: every cell is the target of at most one window
    return dx.reshape(C, H, W)


def gather_pool2x2(a, route):
    """a [C,H,W] tensor, route [C,Ho,Wo] -> [C,Ho,Wo]: the pool as a gather (a window routed nowhere gives 0)"""
    C = a.shape[0]
    idx = torch.as_tensor(np.asarray(route), dtype=torch.long)
    g = torch.gather(a.reshape(C, -1), 1, idx.clamp(min=0).reshape(C, -1)).reshape(idx.shape)
    return torch.where(idx >= 0, g, torch.zeros((), dtype=a.dtype))


class Trainer(TC.Trainer):
    """train_conv_np.Trainer on the WHOLE trunk: conv = [(w, b)] of all its conv layers, pool_after[l] true where layer l is followed by
    the pool; the last trunk_layers of them are trained (the parent's depth = 2 + trunk_layers with K = len(conv))."""

    def __init__(self, P, conv, pool_after, trunk_layers, momentum, weight_decay, **kw):
        super().__init__(P, conv, 2 + trunk_layers, momentum, weight_decay, **kw)
        self.pool_after = [bool(v) for v in pool_after]
        assert len(self.pool_after) == self.K and 1 <= self.k < self.K

    def block(self, a0, masks=None, routes=None):
        """the k trained layers on the saved input map a0 of the first of them.  masks[j]: bool [C,h,w] of the j-th trained layer's
        output BEFORE its pool (None: relu); routes[j]: the routing of that layer's pool (ignored where the layer has none; routes None
        or routes[j] None: the first maximum of the float side's own map) -> the last layer's output"""
        a = torch.as_tensor(np.asarray(a0)).to(self.dtype)[None]
        for j in range(self.k):
            l = self.K - self.k + j
            a = torch.nn.functional.conv2d(a, self.cw[l], self.cb[l], padding=1)
            a = torch.relu(a) if masks is None else a * torch.as_tensor(np.asarray(masks[j])).to(self.dtype)[None]
            if self.pool_after[l]:
                r = None if routes is None else routes[j]
                a = gather_pool2x2(a[0], first_max_route(a[0].detach().numpy()) if r is None else r)[None]
        return a[0]

    def step(self, x, rois, gt, labels, images, lr, PH=7, PW=7, scale=0.25):
        """as the parent's; images: [(a0, masks or None, argmax or None, rois5, routes or None)]"""
        for gr in self.opt.param_groups:
            gr["lr"] = lr
        self.opt.zero_grad()
        xt = torch.as_tensor(np.asarray(x)).to(self.dtype).clone().requires_grad_(True)
        L_cls, L_box = self.head(xt, rois, gt, labels)
        (L_cls + L_box).backward()
        dx6 = xt.grad.detach()
        row = 0
        for a0, masks, argmax, rois5, routes in images:
            n = len(rois5)
            top = self.block(a0, masks, routes)
            am = TC.own_argmax(top.detach().numpy(), rois5, PH, PW, scale) if argmax is None else argmax
            pooled = TC.gather_pool(top, am)
            pooled.backward(dx6[row:row + n].reshape(pooled.shape))
            row += n
        self.opt.step()
        return (float(L_cls.detach()), float(L_box.detach())), dx6.numpy()
