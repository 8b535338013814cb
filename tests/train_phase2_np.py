"""Restatements for MultiPathNet's conv5 block trained through the skip pooling (test infrastructure; include/mpn.h
mpn_mpnet_train_begin_conv): tests/train_towers_np.py extended BELOW the towers' operands.

Trainer is the step by PyTorch-CPU autograd in a chosen dtype: the conv block rebuilt from its saved input map (ReLUs as GIVEN masks, or
its own), per tower a gather of the block's output at a GIVEN argmax (or a max over each Foveal window of its own), nn.Normalize(2) x 1000
with the 1e-10 inside the root, the conv4 / conv3 slabs of the operand as constants, then the towers and losses of
train_towers_np.torch_steps, with the trained conv tensors in the same torch.optim.SGD.  In float64 it is the reference, in float32 the
yardstick.  Beside it, in numpy fp32, one add at a time: the gradient map's chain (item 4 of the contract) and nn.Normalize's backward
in its stated summation order (item 2), with the bound that order gives against float64."""
import numpy as np
import torch

import train_conv_np as TC
import train_towers_np as TT

U = 2.0 ** -24
F32 = np.float32
NORM_THREADS = 256   # train.h kNormBwdThreads
MUL = 1000.0
REGION_OFF = (0.25, 0.5, 1.5)   # modules/Foveal.lua: x - w * off, w * mul
REGION_MUL = (1.5, 2.0, 4.0)


# ---- the inputs of tests/test_gpu_train_phase2.py (tests/test_train_phase2_cpu.py checks the edge cases they hold) ----
H, W, MAXR, PP, NT, SCALE = 150, 250, 200, 49, 5, 1.0 / 16
REGIONS = (0, 1, 2, 3, 1)   # models.MPN_TOWERS' Foveal regions
STD, MEAN = [0.1, 0.1, 0.2, 0.2], [0.0, 0.0, 0.0, 0.0]   # models.synthetic_params' BBoxNorm statistics
NETS = {
    "B": dict(cfg=[8, 16, "P", 16, 24, "P", 24, 24, "P", 40, "P", 48], c5=48, fc=256, C=7, K=1, k=1, layers=[7]),
    "C": dict(cfg=[8, 16, "P", 16, 24, "P", 24, 24, "P", 40, "P", 48, 12, 48], c5=48, fc=128, C=5, K=2, k=3, layers=[7, 8, 9]),
    # a last layer of 44 channels: a handle refuses such a trunk (feat_c % 8), tests/test_gpu_train_phase2.py asserts the refusal
    "D": dict(cfg=[8, 16, "P", 16, 24, "P", 24, 24, "P", 40, "P", 44], c5=44, fc=128, C=5, K=1, k=1, layers=[7]),
}
GRAD_BATCHES = {"B70_two_images": [(33, 9), (37, 11)], "B128_one_image": [(128, 40)], "B1": [(1, 0)]}
_params = {}


def params(name):
    from multipathnet_amd import models
    if name not in _params:
        c = NETS[name]
        _params[name] = models.synthetic_mpnet_params(c["cfg"], pooled=7, fc_dim=c["fc"], n_classes=c["C"], n_integral=c["K"], seed=557)
    return _params[name]


def batch(seed, n, C, n_bg):
    return TT.make_batch(seed, n, C, n_bg, H, W)


def grad_parts(name, case):
    c = NETS[name]
    if case == "B1":   # one foreground row with a near GT box
        return [tuple(a[1:2] if j else a for j, a in enumerate(batch(1234, 2, c["C"], 0)))]
    return [batch(1000 + 17 * i + c["fc"], n, c["C"], n_bg) for i, (n, n_bg) in enumerate(GRAD_BATCHES[case])]


def map_size(cfg, l, h=H, w=W):
    """the size of conv layer l's output (before its own pool) for an h x w image: halved, rounding up, at every pool below it"""
    convs = -1
    for item in cfg:
        if item == "P":
            if convs < l:
                h, w = (h + 1) // 2, (w + 1) // 2
        else:
            convs += 1
    return h, w


def has_zero_tie(top, rois5, own, scale=SCALE):
    """is there a (row, channel, bin) whose window has several cells, none above 0 and at least two equal to 0 — the first-maximum tie?"""
    top = np.asarray(top)
    win = TC.roi_windows(rois5, top.shape[1], top.shape[2], 7, 7, scale)
    for n, row in enumerate(win):
        for b, (hs, he, ws, we) in enumerate(row):
            if (he - hs) * (we - ws) < 2 or he <= hs or we <= ws:
                continue
            sub = top[:, hs:he, ws:we].reshape(top.shape[0], -1)
            if ((sub.max(1) == 0) & ((sub == 0).sum(1) >= 2)).any():
                return True
    return False


def project(boxes, scale=1.0):
    """mpn_project_im_rois in fp32: [n,4] boxes of the image -> [n,5] rows (1, (v - 1) * scale + 1)"""
    b = np.asarray(boxes, F32)
    out = np.ones((len(b), 5), F32)
    out[:, 1:] = ((b + F32(-1.0)) * F32(scale) + F32(1.0)).astype(F32)
    return out


def foveal(rois5):
    """mpn_foveal_forward: [n,5] -> [n,4,5], region 0 the box itself, regions 1..3 grown about its centre (double arithmetic, one rounding)"""
    r = np.asarray(rois5, F32)
    out = np.empty((len(r), 4, 5), F32)
    out[:, 0] = r
    x, y, x2, y2 = (r[:, i].astype(np.float64) for i in (1, 2, 3, 4))
    w, h = x2 - x, y2 - y
    for k in range(3):
        xx, yy = x - w * REGION_OFF[k], y - h * REGION_OFF[k]
        out[:, k + 1, 0] = r[:, 0]
        out[:, k + 1, 1], out[:, k + 1, 2] = xx.astype(F32), yy.astype(F32)
        out[:, k + 1, 3], out[:, k + 1, 4] = (xx + w * REGION_MUL[k]).astype(F32), (yy + h * REGION_MUL[k]).astype(F32)
    return out


# ---- item 4: the gradient map's chain ----
def g5_chain(dx, argmax, regions, row0, rows, top):
    """dx [T][B, c5, PP] fp32, argmax {region: [B, c5, PP] int}, regions [T] the towers' regions, the image's rows [row0, row0 + rows),
    top [c5, h, w] the block's output -> [c5, h, w] fp32: per cell ONE chain from +0.0, towers ascending, rows ascending, bins ascending,
    one fp32 add per term, then the mask [top > 0].  (Channels are walked together: a channel's cells are its own.)"""
    c5, h, w = top.shape
    out = np.zeros((c5, h * w), F32)
    ch = np.arange(c5)
    for t, r in enumerate(regions):
        g, am = np.asarray(dx[t], F32), np.asarray(argmax[r]).astype(np.int64)
        for n in range(row0, row0 + rows):
            for b in range(g.shape[2]):
                i = am[n, :, b]
                ok = i >= 0
                out[ch[ok], i[ok]] = (out[ch[ok], i[ok]] + g[n, ok, b]).astype(F32)
    return np.where(np.asarray(top).reshape(c5, -1) > 0, out, F32(0)).reshape(c5, h, w)


# ---- item 2: nn.Normalize(2) x mul backward ----
def normalize_backward64(x, y, g, mul=MUL):
    """the closed form in float64 on [B, c5, PP] arrays: s = mul / sqrt(sum x^2 + 1e-10), dx = s (g - y (y . g) / mul^2)"""
    x, y, g = (np.asarray(a, np.float64) for a in (x, y, g))
    s = mul / np.sqrt((x * x).sum((1, 2)) + 1e-10)
    d = (y * g).sum((1, 2))
    return s[:, None, None] * (g - y * (d / (mul * mul))[:, None, None])


def norm_entries(C, PP):
    """E = ceil(C / 8) * PP * 8: the entries both sums walk (the slab's records times 8 lanes, pad lanes of the last channel block counted)"""
    return -(-C // 8) * PP * 8


def _entry_order(a):
    """[B, C, PP] -> ([B, L, 256] values, [L, 256] bool `real`): entry e = (c / 8 * PP + bin) * 8 + c % 8 at [e / 256, e % 256], e <
    ceil(C / 8) * PP * 8.  `real` is False at the pad lanes of the last channel block (c >= C) and behind the last entry: those are
    SKIPPED by _fma_sum, not added as zeros (fma(0, 0, acc) would give the same bits; the kernel's `continue` is what is restated)."""
    B, C, PP = a.shape
    Cb = -(-C // 8)
    full = np.zeros((B, Cb * 8, PP), a.dtype)
    full[:, :C] = a
    e = full.reshape(B, Cb, 8, PP).transpose(0, 1, 3, 2).reshape(B, -1)
    ok = np.broadcast_to((np.arange(Cb * 8) < C).reshape(Cb, 1, 8), (Cb, PP, 8)).reshape(-1)
    assert e.shape[1] == norm_entries(C, PP)
    L = -(-e.shape[1] // NORM_THREADS)
    pad, real = np.zeros((B, L * NORM_THREADS), a.dtype), np.zeros(L * NORM_THREADS, bool)
    pad[:, :e.shape[1]], real[:e.shape[1]] = e, ok
    return pad.reshape(B, L, NORM_THREADS), real.reshape(L, NORM_THREADS)


def _fma_sum(a, b):
    """the stated order: 256 partial sums, partial t over the entries t, t + 256, .. ascending with one fused multiply-add each, then the
    tree.  The product of two fp32 values is exact in float64; the float64 sum product + partial is then rounded to fp32.  For operands
    of full mantissa that is the fma only up to a double rounding (test_train_phase2_kernels_ref_cpu.py shows a counter-example); for
    operands of at most 12 significant bits in [2^-6, 2^3] (bit_exact_draw) the float64 sum is exact and this IS the fma."""
    (A, real), (Bv, _) = _entry_order(np.asarray(a, F32)), _entry_order(np.asarray(b, F32))
    A, Bv = A.astype(np.float64), Bv.astype(np.float64)
    part = np.zeros((A.shape[0], NORM_THREADS), F32)
    for l in range(A.shape[1]):
        part = np.where(real[l][None, :], (A[:, l] * Bv[:, l] + part.astype(np.float64)).astype(F32), part)
    h = NORM_THREADS // 2
    while h >= 1:
        part = (part[:, :h] + part[:, h:2 * h]).astype(F32)
        h //= 2
    return part[:, 0]


def normalize_backward_f32(x, y, g, mul=MUL):
    """train.h normalize_backward_c8 in numpy fp32, operation by operation"""
    x, y, g = (np.asarray(a, F32) for a in (x, y, g))
    return normalize_backward_tail(_fma_sum(x, x), _fma_sum(y, g), y, g, mul)


def normalize_backward_tail(ss, d, y, g, mul=MUL):
    """what the kernel does with its two sums ss = sum x^2 and d = sum y g ([B] fp32), operation by operation"""
    ss, d, y, g = (np.asarray(a, F32) for a in (ss, d, y, g))
    s = (F32(mul) / np.sqrt((ss + F32(1e-10)).astype(F32)).astype(F32)).astype(F32)
    coef = (d / F32(F32(mul) * F32(mul))).astype(F32)
    inner = (g - (y * coef[:, None, None]).astype(F32)).astype(F32)
    return (s[:, None, None] * inner).astype(F32)


def normalize_backward_bound(x, y, g, mul=MUL):
    """Elementwise bound of |fp32 result - normalize_backward64| for fp32 inputs, from the stated order.  With E = ceil(C / 8) * PP * 8
    entries (pad lanes counted: they take a slot of the walk, though no rounding) a partial sum is a chain of at most L = ceil(E / 256)
    fused multiply-adds and the tree adds 8 levels, so each sum carries at most L + 8
    roundings: the sum of squares (all terms >= 0) a relative error (L + 8) u, the dot product an absolute error (L + 8) u sum|y g|.
      s:     (L + 8) u / 2 through the root, + u for the 1e-10 add, + u for the root, + u for the division        =: es (relative)
      coef:  D / mul^2, mul^2 exact, one division: relative u on top of D's absolute error dD = (L + 8) u sum|y g|
      inner: g - y coef: the product's u and the subtraction's u; dx = s * inner: u.
    |dx - dx64| <= (es + 2u) |dx64| + s |y| (2u |D| + dD) / mul^2, times 1.01 for the second-order terms."""
    x, y, g = (np.asarray(a, np.float64) for a in (x, y, g))
    L = -(-norm_entries(x.shape[1], x.shape[2]) // NORM_THREADS)
    n = L + 8
    s = mul / np.sqrt((x * x).sum((1, 2)) + 1e-10)
    D, aD = (y * g).sum((1, 2)), np.abs(y * g).sum((1, 2))
    dx = np.abs(normalize_backward64(x, y, g, mul))
    es = (n / 2.0 + 3.0) * U
    tail = s[:, None, None] * np.abs(y) * ((2 * U * np.abs(D) + n * U * aD) / (mul * mul))[:, None, None]
    return 1.01 * ((es + 2 * U) * dx + tail)


# ---- the step by autograd ----
def conv_names(layers):
    return ["conv_w.%d" % l for l in layers] + ["conv_b.%d" % l for l in layers]


class Trainer(object):
    """P: train_towers_np's flat dict; conv {l: (w [Cout,Cin,3,3], b [Cout])} of the trained layers l (trunk indices, ascending)."""

    def __init__(self, P, conv, K, momentum, weight_decay, bbox_weight=1.0, mean=None, std=None, dtype=torch.float64, lr=1.0, norm=True,
                 pooled=7, scale=1.0 / 16):
        self.dtype, self.K, self.bbox_weight, self.mean, self.std, self.norm = dtype, K, bbox_weight, mean, std, norm
        self.PH, self.scale = pooled, scale
        self.nt = TT.n_towers_of(P)
        self.layers = sorted(conv)
        mk = lambda a: torch.as_tensor(np.asarray(a)).to(dtype).clone().requires_grad_(True)
        self.Pt = {n: mk(P[n]) for n in TT.names(self.nt)}
        for l in self.layers:
            self.Pt["conv_w.%d" % l], self.Pt["conv_b.%d" % l] = mk(conv[l][0]), mk(conv[l][1])
        self.opt = torch.optim.SGD([{"params": [v for n, v in self.Pt.items() if n.endswith("_w") or n.startswith("conv_w")], "weight_decay": weight_decay},
                                    {"params": [v for n, v in self.Pt.items() if not (n.endswith("_w") or n.startswith("conv_w"))], "weight_decay": 0.0}],
                                   lr=lr, momentum=momentum)

    def block(self, a0, masks=None):
        a = torch.as_tensor(np.asarray(a0)).to(self.dtype)[None]
        for j, l in enumerate(self.layers):
            a = torch.nn.functional.conv2d(a, self.Pt["conv_w.%d" % l], self.Pt["conv_b.%d" % l], padding=1)
            a = torch.relu(a) if masks is None else a * torch.as_tensor(np.asarray(masks[j])).to(self.dtype)[None]
        return a[0]

    def operands(self, images, regions, rest):
        """images [(a0, masks or None, {region: argmax} or None, fov [n,4,5])] in train_add order; rest [T][B, Kcat_t - c5, PP] the conv4 /
        conv3 slabs (constants) -> xs [T][B, Kcat_t, PP] tensors"""
        slabs = [[] for _ in regions]
        for a0, masks, argmax, fov in images:
            top = self.block(a0, masks)
            own = {}
            for t, r in enumerate(regions):
                if argmax is not None:
                    am = argmax[r]
                else:
                    if r not in own:
                        own[r] = TC.own_argmax(top.detach().numpy(), fov[:, r], self.PH, self.PH, self.scale)
                    am = own[r]
                x = TC.gather_pool(top, am)
                if self.norm:
                    x = x / torch.sqrt((x * x).sum((1, 2), keepdim=True) + 1e-10) * MUL
                slabs[t].append(x)
        return [torch.cat([torch.cat(slabs[t], 0), torch.as_tensor(np.asarray(rest[t])).to(self.dtype)], 1) for t in range(len(regions))]

    def step(self, images, regions, rest, rois, gt, labels, lr, k=0, drop=None):
        """one step -> ((L_cls, L_box), {name: gradient before weight decay})"""
        dtype, Pt, nt = self.dtype, self.Pt, self.nt
        for gr in self.opt.param_groups:
            gr["lr"] = lr
        xs = self.operands(images, regions, rest)
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
            tg = torch.stack([(xtc - xc) / w, (ytc - yc) / h, torch.log(wt / w), torch.log(ht / h)], 1)
            if self.std is not None and self.std[0] != 0:
                tg = (tg - torch.tensor(list(self.mean), dtype=dtype)) / torch.tensor(list(self.std), dtype=dtype)
            cols = 4 * y[fg][:, None] + torch.arange(4)[None, :]
            L_box = self.bbox_weight * torch.nn.SmoothL1Loss(reduction="sum")(that[fg[:, None], cols], tg) / B
        self.opt.zero_grad()
        (L_cls + L_box).backward()
        for p_ in Pt.values():      # a tensor the loss does not reach (a classifier not selected) still takes its step
            if p_.grad is None:
                p_.grad = torch.zeros_like(p_)
        G = {n: v.grad.detach().numpy().copy() for n, v in Pt.items()}
        self.opt.step()
        return (float(L_cls.detach()), float(L_box.detach())), G

    def params(self):
        return {n: v.detach().numpy() for n, v in self.Pt.items()}
