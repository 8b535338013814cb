"""numpy restatements of the detection head's score and box operations (boxes.hip, pipeline.hip, nms.hip's bbox_vote): a float64 version of each,
and for the order-sensitive ones a sequential fp32 emulation of the documented order (every fp32 numpy operation rounds on its own, so nothing can
contract into an FMA).  tests/test_boxes_ref_cpu.py checks them against the CPU oracle on the GPU tests' own shape lists (the lists live here);
tests/test_gpu_box_kernels_numerics.py compares the kernels with them."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24  # fp32 unit roundoff
TINY = 2.0 ** -126  # smallest normal fp32

# ---- the shape lists shared by the CPU check of this file and the GPU tests --------------------------------------------------
SOFTMAX_M = (1, 3, 4, 5, 37)
SOFTMAX_C = (1, 2, 21, 63, 64, 65, 81, 128, 129, 255, 256)
SOFTMAX_C_FREE = SOFTMAX_C + (257, 1000)  # mpn_softmax_forward has no C limit
SOFTMAX_K = (1, 2, 6, 8)
SOFTMAX_SIGMA = (1.0, 5.0, 40.0)
DECODE_N = (1, 2, 255, 256, 257)
DECODE_C = (1, 2, 21, 81)
MERGE_MC = ((1, 1), (255, 1), (1, 256), (257, 1), (37, 21))  # (M, C): M*C = 1, 255, 256, 257, 21*37
SELECT_N = (1, 255, 256, 257, 513, 1000)
SELECT_C = (2, 21, 81)
VOTE_N_NMS = (1, 63, 64, 65, 130)
VOTE_M = (1, 255, 256, 257, 600)
VOTE_POW = (1.0, 0.5, 2.0)
SCALE_PAIRS = ((1, 5), (2, 3), (7, 8), (8, 7), (64, 65), (65, 64), (3, 1), (100, 1), (600, 1000), (1000, 600), (999, 333), (1000, 999), (480, 600),
               (37, 37))
COMPANION_N = (0, 1, 255, 256, 257)


def scale_cases():
    """(H, W, H2, W2, C): every pair of SCALE_PAIRS once on each axis, the two axes of a case taking different pairs"""
    P = SCALE_PAIRS
    return [(P[i][0], P[(i + 5) % len(P)][0], P[i][1], P[(i + 5) % len(P)][1], 1 + 2 * (i % 2)) for i in range(len(P))]


def logits(rng, M, C, sigma):
    return (rng.standard_normal((M, C)) * sigma).astype(F32)


def rois(rng, n, W=1000, H=600):
    c = rng.uniform([1, 1], [W, H], (n, 2))
    wh = np.exp(rng.uniform(np.log(4), np.log(600), (n, 2)))
    return np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 1, [W, H, W, H]).astype(F32)


def vote_tables(rng, m, span=260.0, lo=40.0, hi=160.0):
    """a scored table whose boxes overlap heavily (many voters per kept box): [m, 5] fp32, scores in (0, 1)"""
    c = rng.uniform(0, span, (m, 2))
    wh = np.exp(rng.uniform(np.log(lo), np.log(hi), (m, 2)))
    return np.concatenate([c - wh / 2, c + wh / 2, rng.uniform(0.01, 1, (m, 1))], 1).astype(F32)


# ---- softmax -----------------------------------------------------------------------------------------------------------------
def softmax_shift(x):
    """d = fl32(x - rowmax): the documented order's fp32 subtraction, exactly reproducible (fmaxf ignores a NaN; a row of NaNs keeps -inf)."""
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        mx = np.fmax.reduce(x, axis=-1, initial=F32(-np.inf), keepdims=True).astype(F32)
        return (x - mx).astype(F32)


def softmax(x):
    """float64 exp(d) / sum exp(d) over the last axis, d = fl32(x - max).  inf / NaN follow IEEE: a NaN anywhere, a +inf (inf - inf) or a row
    of -inf makes the sum NaN and so the whole row NaN; a -inf among finite values gives exactly 0 there."""
    d = softmax_shift(x).astype(F64)
    with np.errstate(all="ignore"):
        e = np.exp(d)
        return e / e.sum(-1, keepdims=True)


def softmax_f32(x):
    """the oracle's chain in fp32: e = expf(d) (numpy's), serial sum in column order, e / sum"""
    d = softmax_shift(x)
    with np.errstate(all="ignore"):
        e = np.exp(d).astype(F32)
        s = np.zeros(e.shape[:-1], F32)
        for c in range(e.shape[-1]):
            s = (s + e[..., c]).astype(F32)
        return (e / s[..., None]).astype(F32)


def softmax_mean(x):
    """K-way softmax mean (model_utils.lua:296-313): x [M, K, C] -> float64 [M, C]"""
    with np.errstate(all="ignore"):
        return softmax(x).sum(1) / x.shape[1]


def mean_over_k_f32(p):
    """nn.Mean in fp32 on fp32 probabilities p [M, K, C]: sum in k order, then * fl32(1 / K)"""
    p = np.asarray(p, F32)
    s = np.zeros((p.shape[0], p.shape[2]), F32)
    with np.errstate(all="ignore"):
        for k in range(p.shape[1]):
            s = (s + p[:, k]).astype(F32)
        return (s * (F32(1) / F32(p.shape[1]))).astype(F32)


def softmax_bound(C, K=None):
    """relative error bound per element, see tests/test_gpu_box_kernels_numerics.py"""
    b = 11 + math.ceil(C / 64)
    return (b + (K + 1 if K is not None else 0)) * U


# ---- BBoxNorm + convertFrom + clamp ------------------------------------------------------------------------------------------
def norm_f32(d, mean4, std4):
    """BBoxNorm.lua:28-29 in fp32: d * std, then + mean, each rounded; d [N, 4C]"""
    d = np.asarray(d, F32)
    s, m = np.tile(np.asarray(std4, F32), d.shape[1] // 4), np.tile(np.asarray(mean4, F32), d.shape[1] // 4)
    with np.errstate(all="ignore"):
        return ((d * s).astype(F32) + m).astype(F32)


def _split(boxes, deltas, dt):
    b = np.asarray(boxes, dt).reshape(-1, 1, 4)
    d = np.asarray(deltas, dt).reshape(b.shape[0], -1, 4)
    return b, d


def _c64(v):
    return np.asarray(v, F32).astype(F64)


def decode(boxes, deltas, mean4=None, std4=None):
    """float64 BBoxNorm + convertFrom (utils.lua:229-247): boxes [N, 4], deltas [N, 4C] -> [N, 4C]"""
    b, d = _split(boxes, deltas, F64)
    if std4 is not None:
        d = d * _c64(std4) + _c64(mean4)  # the constants are the fp32 ones the device receives
    with np.errstate(all="ignore"):
        xc, yc = (b[..., 0] + b[..., 2]) * 0.5, (b[..., 1] + b[..., 3]) * 0.5
        w, h = b[..., 2] - b[..., 0], b[..., 3] - b[..., 1]
        xt, yt = xc + d[..., 0] * w, yc + d[..., 1] * h
        hw, hh = np.exp(d[..., 2]) * w * 0.5, np.exp(d[..., 3]) * h * 0.5
        return np.stack([xt - hw, yt - hh, xt + hw, yt + hh], -1).reshape(b.shape[0], -1)


def decode_f32(boxes, deltas):
    """convertFrom in the documented fp32 order with numpy's expf (bit-equal to the oracle wherever the two expf agree, as at dw = dh = 0)"""
    b, d = _split(boxes, deltas, F32)
    h5 = F32(0.5)
    with np.errstate(all="ignore"):
        xc, yc = (b[..., 0] + b[..., 2]) * h5, (b[..., 1] + b[..., 3]) * h5
        w, h = b[..., 2] - b[..., 0], b[..., 3] - b[..., 1]
        xt, yt = xc + d[..., 0] * w, yc + d[..., 1] * h
        hw, hh = (np.exp(d[..., 2]).astype(F32) * w) * h5, (np.exp(d[..., 3]).astype(F32) * h) * h5
        return np.stack([xt - hw, yt - hh, xt + hw, yt + hh], -1).astype(F32).reshape(b.shape[0], -1)


def decode_bound(boxes, deltas, mean4=None, std4=None):
    """first-order absolute error bound of the fp32 chain against decode(), per output element (derivation: the GPU test module's docstring)"""
    b, d0 = _split(boxes, deltas, F64)
    d = d0 if std4 is None else d0 * _c64(std4) + _c64(mean4)
    dd = np.zeros_like(d) if std4 is None else (np.abs(d0 * _c64(std4)) + np.abs(d)) * U  # absolute error of a normed delta
    out = decode(boxes, deltas, mean4, std4).reshape(d.shape)
    res = np.empty_like(out)
    for ax in (0, 1):
        lo, hi = b[..., ax], b[..., ax + 2]
        w = hi - lo
        xt = (lo + hi) * 0.5 + d[..., ax] * w
        hw = np.exp(d[..., ax + 2]) * w * 0.5
        common = np.abs(lo + hi) + 2 * np.abs(d[..., ax] * w) + np.abs(xt) + 4 * np.abs(hw)
        common = common * U + dd[..., ax] * np.abs(w) + dd[..., ax + 2] * np.abs(hw)
        for k in (ax, ax + 2):
            res[..., k] = (common + np.abs(out[..., k]) * U) * (1 + 16 * U)  # second-order terms
    return res.reshape(out.shape[0], -1)


def clamp(bbox, im_w, im_h):
    """Tester_FRCNN.lua:75-78 on (x, y) pairs as the `<` / `>` chain applies it: v < 1 -> 1, v > hi -> hi, anything else (a NaN too) unchanged"""
    v = np.asarray(bbox, F32).copy().reshape(-1, 2)
    for col, hi in ((0, F32(im_w)), (1, F32(im_h))):
        x = v[:, col].copy()
        with np.errstate(all="ignore"):
            v[:, col] = np.where(x < F32(1), F32(1), np.where(x > hi, hi, x))
    return v.reshape(np.asarray(bbox).shape)


# ---- the flip merge ----------------------------------------------------------------------------------------------------------
def merge(sA, bA, sB, bB, im_w):
    """float64 merge of the two halves (rule 4), unclamped: scores [M, C], boxes [M, 4C]"""
    sA, bA, sB, bB = (np.asarray(t, F64) for t in (sA, bA, sB, bB))
    q = bB.reshape(-1, 4)
    back = np.stack([im_w - q[:, 2] + 1, q[:, 1], im_w - q[:, 0] + 1, q[:, 3]], 1).reshape(bB.shape)
    return (sA + sB) * 0.5, (bA + back) * 0.5


# ---- bbox_vote ---------------------------------------------------------------------------------------------------------------
def overlap_f32(s, k):
    """nms.c:14-41 in fp32: s [m, 4+] against k [n, 4+] -> [n, m]"""
    s, k = np.asarray(s, F32)[None, :, :], np.asarray(k, F32)[:, None, :]
    one = F32(1)
    with np.errstate(all="ignore"):
        x1, y1 = np.where(s[..., 0] > k[..., 0], s[..., 0], k[..., 0]), np.where(s[..., 1] > k[..., 1], s[..., 1], k[..., 1])
        x2, y2 = np.where(s[..., 2] < k[..., 2], s[..., 2], k[..., 2]), np.where(s[..., 3] < k[..., 3], s[..., 3], k[..., 3])
        w, h = (x2 - x1) + one, (y2 - y1) + one
        inter = w * h
        sa = ((s[..., 2] - s[..., 0]) + one) * ((s[..., 3] - s[..., 1]) + one)
        ka = ((k[..., 2] - k[..., 0]) + one) * ((k[..., 3] - k[..., 1]) + one)
        iou = inter / ((sa + ka) - inter)
        return np.where((w <= 0) | (h <= 0), F32(0), iou).astype(F32)


def pow_scores(scored, score_pow):
    """Tester_FRCNN.lua:119-121 as THFloatTensor_pow does it: C pow on the score promoted to double, rounded to float once; pow == 1: untouched"""
    sb = np.asarray(scored, F32).copy()
    if float(score_pow) != 1.0:
        with np.errstate(all="ignore"):
            sb[:, 4] = np.power(sb[:, 4].astype(F64), F64(F32(score_pow))).astype(F32)
    return sb


def vote_f32(nms_boxes, scored, thr, score_pow=1.0):
    """nms.c:110-142 in fp32, the voters in j order: [n, 5]"""
    nb, sb = np.asarray(nms_boxes, F32).reshape(-1, 5), pow_scores(np.asarray(scored, F32).reshape(-1, 5), score_pow)
    take = overlap_f32(sb, nb) > F32(thr)
    acc = np.zeros((nb.shape[0], 5), F32)
    with np.errstate(all="ignore"):
        for j in range(sb.shape[0]):
            t = take[:, j]
            for f in range(4):
                acc[t, f] = (acc[t, f] + sb[j, f] * sb[j, 4]).astype(F32)
            acc[t, 4] = (acc[t, 4] + sb[j, 4]).astype(F32)
        out = np.concatenate([(acc[:, :4] / acc[:, 4:5]).astype(F32), nb[:, 4:5]], 1)
    return out


def vote(nms_boxes, scored, thr, score_pow=1.0):
    """the same vote with float64 sums over the voters the fp32 overlap admits (the weights are the fp32 pow'd scores).  Returns ([n, 5], the
    absolute bound [n, 4] of a sequential fp32 sum against it): with v voters the numerator carries one rounding per product and v - 1 per
    sum (v + 1 with the first-order slack, on sum|x s|), the denominator v - 1 on sum|s|, the quotient one:
    ((v + 1) * sum|x s| / |sum s| + ((v - 1) * sum|s| / |sum s| + 1) * |res|) * 2^-24; with weights of one sign sum|s| = |sum s|."""
    nb, sb = np.asarray(nms_boxes, F32).reshape(-1, 5), pow_scores(np.asarray(scored, F32).reshape(-1, 5), score_pow)
    take = (overlap_f32(sb, nb) > F32(thr)).astype(F64)
    s = sb[:, 4].astype(F64)
    with np.errstate(all="ignore"):
        den = take @ s
        num = take @ (sb[:, :4].astype(F64) * s[:, None])
        absnum = take @ np.abs(sb[:, :4].astype(F64) * s[:, None])
        res = num / den[:, None]
        v = take.sum(1)[:, None]
        absden = (take @ np.abs(s))[:, None]
        aden = np.abs(den)[:, None]
        bound = ((v + 1) * absnum / aden + ((v - 1) * absden / aden + 1) * np.abs(res)) * U * (1 + 16 * U)
    return np.concatenate([res, nb[:, 4:5].astype(F64)], 1), bound


# ---- image.scale: the two-pass 1-D resample ----------------------------------------------------------------------------------
def _line_index(slen, dlen):
    """the fp32 index arithmetic of one line (what the kernel computes): upscale -> (si, sf); downscale -> (i0, i1, f0, f1)"""
    d = np.arange(dlen)
    if dlen > slen:
        scale = F32(slen - 1) / F32(dlen - 1)
        sf = (d.astype(F32) * scale).astype(F32)
        si = sf.astype(np.int64)
        return si, (sf - si.astype(F32)).astype(F32)
    scale = F32(slen) / F32(dlen)
    s0, s1 = (d.astype(F32) * scale).astype(F32), ((d + 1).astype(F32) * scale).astype(F32)
    i0, i1 = s0.astype(np.int64), s1.astype(np.int64)
    return i0, i1, (s0 - i0.astype(F32)).astype(F32), (s1 - i1.astype(F32)).astype(F32)


def scale_line(src, dlen, dt=F64):
    """one 1-D pass along the LAST axis (torch/image scaleLinear_rowcol's published rule), in dt = float64 (indices and fractions still the
    fp32 ones) or in dt = float32 (the kernel's order, every step rounded)"""
    src = np.asarray(src, dt)
    slen = src.shape[-1]
    one = dt(1)
    if dlen == slen:
        return src.copy()
    out = np.empty(src.shape[:-1] + (dlen,), dt)
    if dlen > slen:
        if slen == 1:
            out[...] = src[..., :1]
            return out
        si, sf = _line_index(slen, dlen)
        si, sf = si[:-1], sf[:-1].astype(dt)
        out[..., :-1] = ((one - sf) * src[..., si]).astype(dt) + (sf * src[..., si + 1]).astype(dt)
        out[..., -1] = src[..., -1]
        return out.astype(dt)
    i0, i1, f0, f1 = _line_index(slen, dlen)
    for d in range(dlen):
        a, b = int(i0[d]), int(i1[d])
        acc = ((one - dt(f0[d])) * src[..., a]).astype(dt)
        n = one - dt(f0[d])
        for i in range(a + 1, b):
            acc = (acc + src[..., i]).astype(dt)
            n = dt(n + one)
        if b < slen and b > a:
            acc = (acc + (dt(f1[d]) * src[..., b]).astype(dt)).astype(dt)
            n = dt(n + dt(f1[d]))
        out[..., d] = acc / n
    return out.astype(dt)


def image_scale(im, H2, W2, dt=F64):
    """rows first ([C, H, W] -> [C, H, W2]), then columns (-> [C, H2, W2]); dt = F32 keeps the fp32 intermediate the kernel keeps"""
    t = scale_line(np.asarray(im, dt), W2, dt)
    return np.ascontiguousarray(np.swapaxes(scale_line(np.swapaxes(t, 1, 2), H2, dt), 1, 2))


def scale_pass_bound(slen, dlen):
    """relative bound of one fp32 pass on a non-negative line, in units of 2^-24.  Upscale: 1 - sf, two products, one sum: 3.  Downscale over
    n = i1 - i0 + 1 <= ceil(slen / dlen) + 1 taps: the weights 1 - f0 and f1 (1 each), the products (1), n - 1 sums of the numerator and of the
    count, the quotient: 2n + 2 at most."""
    if dlen == slen or slen == 1:
        return 0
    return 3 if dlen > slen else 2 * (math.ceil(slen / dlen) + 1) + 2


def image_scale_bound(H, W, H2, W2, amax):
    """absolute bound for a non-negative image with values <= amax: both passes are convex combinations, so the first pass's error reaches the
    output with weight <= 1"""
    return (scale_pass_bound(W, W2) + scale_pass_bound(H, H2)) * U * amax * (1 + 16 * U)
