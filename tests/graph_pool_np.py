"""Plain numpy restatements of the graph executor's pooling, LRN and ROI-pooling ops (test infrastructure).

float64 versions state WHAT each op computes (tests/test_graph_pool_ref_cpu.py checks them against the CPU oracle and PyTorch;
tests/test_gpu_graph_pool_numerics.py checks the HIP kernels against them).  The *_seq32 versions restate the ORDER the average kernels
document: np.float32 adds in row-major order over the in-map cells of the window, then one multiply by float32(1 / (kh * kw)).

The shape lists the GPU tests run are kept here, so the CPU test runs the references over exactly those shapes."""
import numpy as np

# (k, stride, pad, ceil_mode)
MAXPOOL_GEOMS = [(3, 2, 1, 1), (3, 2, 1, 0), (3, 2, 0, 0), (2, 2, 0, 1), (3, 1, 1, 0), (2, 2, 1, 1)]
MAXPOOL_MAPS = [(1, 1), (2, 3), (5, 7), (13, 13), (17, 17)]
MAXPOOL_BATCHES = [1, 3, 37]
# (kh, kw, sh, sw, ph, pw)
AVGPOOL_GEOMS = [(3, 3, 1, 1, 1, 1), (3, 3, 2, 2, 0, 0), (2, 3, 2, 1, 0, 1)]
AVGPOOL_MAPS = [(1, 1), (2, 2), (5, 7), (8, 8), (16, 16), (17, 16)]
LRN_CHANNELS = [5, 8, 13, 24, 96]
LRN_SIZES = [1, 3, 5, 17]
LRN_PARAMS = [(1e-4, 0.75, 1.0), (2e-2, 0.5, 2.0)]
LRN_ROWS = [1, 99, 105]  # B * H * W
ROI_POOLED = [1, 6, 7, 14, 17]
ROI_MAPS = [(1, 1), (2, 37), (9, 3), (38, 63)]
# fused ROI max-pool: (pooled, k, stride, pad)
ROIMAX_GEOMS = [(17, 3, 2, 0), (7, 3, 2, 1), (6, 2, 2, 0), (7, 3, 1, 1)]
ROIMAX_MAPS = [(1, 5), (2, 9), (3, 9), (38, 63)]
GAVG_HW = [1, 36, 49, 64]
GAVG_N = [1, 15, 16, 17, 37]


def pool_out_size(h, k, stride, pad, ceil_mode):
    """floor mode, or ceil mode: round up, but the last window must start inside the padded input (gop_out_dims)"""
    if not ceil_mode:
        return (h + 2 * pad - k) // stride + 1
    o = -(-(h + 2 * pad - k) // stride) + 1
    if pad > 0 and (o - 1) * stride >= h + pad:
        o -= 1
    return o


def _windows(h, k, stride, pad, oh):
    """in-map index range [lo, hi) of each output's window along one axis"""
    return [(max(o * stride - pad, 0), min(o * stride - pad + k, h)) for o in range(oh)]


def maxpool64(x, k, stride, pad, ceil_mode):
    """max over the in-map cells of each window (padded cells never win); NaNs are ignored, a window holding only NaN (or no
    in-map cell) gives -inf.  x [B, C, H, W] -> float64 [B, C, OH, OW]"""
    x = np.asarray(x, np.float64)
    B, C, H, W = x.shape
    OH, OW = pool_out_size(H, k, stride, pad, ceil_mode), pool_out_size(W, k, stride, pad, ceil_mode)
    xs = np.where(np.isnan(x), -np.inf, x)
    y = np.full((B, C, OH, OW), -np.inf)
    for oy, (y0, y1) in enumerate(_windows(H, k, stride, pad, OH)):
        for ox, (x0, x1) in enumerate(_windows(W, k, stride, pad, OW)):
            if y1 > y0 and x1 > x0:
                y[:, :, oy, ox] = xs[:, :, y0:y1, x0:x1].max(axis=(2, 3))
    return y


def avgpool_cells(H, W, kh, kw, sh, sw, ph, pw):
    """number of in-map cells of each window, int [OH, OW]"""
    OH, OW = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    ny = np.array([b - a for a, b in _windows(H, kh, sh, ph, OH)])
    nx = np.array([b - a for a, b in _windows(W, kw, sw, pw, OW)])
    return ny[:, None] * nx[None, :]


def avgpool64(x, kh, kw, sh, sw, ph, pw, bias=None, relu=False):
    """count_include_pad: sum of the in-map cells / (kh * kw), then + bias[c] and ReLU (the commuted pool).  float64"""
    x = np.asarray(x, np.float64)
    B, C, H, W = x.shape
    OH, OW = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    y = np.zeros((B, C, OH, OW))
    for oy, (y0, y1) in enumerate(_windows(H, kh, sh, ph, OH)):
        for ox, (x0, x1) in enumerate(_windows(W, kw, sw, pw, OW)):
            y[:, :, oy, ox] = x[:, :, y0:y1, x0:x1].sum(axis=(2, 3)) / (kh * kw)
    if bias is not None:
        y = y + np.asarray(bias, np.float64)[None, :, None, None]
        if relu:
            y = np.where(y < 0, 0.0, y)
    return y


def avgpool_seq32(x, kh, kw, sh, sw, ph, pw):
    """the average kernels' documented order: fp32 adds from 0 over the in-map cells in row-major order, * float32(1 / (kh * kw))"""
    x = np.asarray(x, np.float32)
    B, C, H, W = x.shape
    OH, OW = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    inv = np.float32(1.0) / np.float32(kh * kw)
    y = np.zeros((B, C, OH, OW), np.float32)
    for oy, (y0, y1) in enumerate(_windows(H, kh, sh, ph, OH)):
        for ox, (x0, x1) in enumerate(_windows(W, kw, sw, pw, OW)):
            acc = np.zeros((B, C), np.float32)
            for iy in range(y0, y1):
                for ix in range(x0, x1):
                    acc = acc + x[:, :, iy, ix]
            y[:, :, oy, ox] = acc * inv
    return y


def lrn64(x, size, alpha, beta, k):
    """out_c = in_c * (k + alpha / size * sum_{|c' - c| <= (size - 1) / 2} in_c'^2) ^ -beta.  float64"""
    x = np.asarray(x, np.float64)
    C = x.shape[1]
    half = (size - 1) // 2
    sq = x * x
    y = np.empty_like(x)
    for c in range(C):
        s = sq[:, max(c - half, 0):min(c + half + 1, C)].sum(axis=1)
        y[:, c] = x[:, c] * (k + alpha / size * s) ** -beta
    return y


def _roundf(v):
    """C roundf of an fp32 value (half away from zero), as int"""
    v = float(np.float32(v))
    return int(np.floor(abs(v) + 0.5)) * (-1 if v < 0 else 1)


def roi_bins(roi, scale, H, W, PH, PW, rule):
    """bin bounds of one ROI row (.., x1, y1, x2, y2), both rules of roi_bin_bounds (coord_offset 1, end_adjust 0), with its fp32
    arithmetic.  Returns (rows, cols): lists of [start, end) per bin; start >= end means an empty bin."""
    f = np.float32
    c = [f(f(f(roi[i]) - f(1.0)) * f(scale)) for i in (1, 2, 3, 4)]
    if rule == 0:
        sw, sh, ew, eh = (_roundf(v) for v in c)
        rw, rh = max(ew - sw + 1, 1), max(eh - sh + 1, 1)
        bh, bw = f(rh) / f(PH), f(rw) / f(PW)
        rows = [(min(max(int(np.floor(f(p) * bh)) + sh, 0), H), min(max(int(np.ceil(f(p + 1) * bh)) + sh, 0), H)) for p in range(PH)]
        cols = [(min(max(int(np.floor(f(p) * bw)) + sw, 0), W), min(max(int(np.ceil(f(p + 1) * bw)) + sw, 0), W)) for p in range(PW)]
        return rows, cols
    x1, y1, x2, y2 = (_roundf(f(v + f(1.0))) - 1 for v in c)
    x1, x2 = min(max(x1, 0), W - 1), min(max(x2, 0), W - 1)
    y1, y2 = min(max(y1, 0), H - 1), min(max(y2, 0), H - 1)
    cw, ch = max(x2 - x1 + 1, 1), max(y2 - y1 + 1, 1)
    rows = [(int(np.floor(f(p * ch) / f(PH))) + y1, int(np.ceil(f((p + 1) * ch) / f(PH))) + y1) for p in range(PH)]
    cols = [(int(np.floor(f(p * cw) / f(PW))) + x1, int(np.ceil(f((p + 1) * cw) / f(PW))) + x1) for p in range(PW)]
    return rows, cols


def roi_pool64(feat, rois, PH, PW, scale, rule):
    """inn.ROIPooling of a one-map feature [C, H, W] -> float64 [N, C, PH, PW]: the max of each bin (NaNs ignored, only-NaN -> -inf),
    an empty bin gives 0"""
    feat = np.asarray(feat, np.float64)
    C, H, W = feat.shape
    fs = np.where(np.isnan(feat), -np.inf, feat)
    rois = np.asarray(rois, np.float32)
    y = np.zeros((rois.shape[0], C, PH, PW))
    for n, r in enumerate(rois):
        rows, cols = roi_bins(r, scale, H, W, PH, PW, rule)
        for i, (y0, y1) in enumerate(rows):
            for j, (x0, x1) in enumerate(cols):
                if y1 > y0 and x1 > x0:
                    y[n, :, i, j] = fs[:, y0:y1, x0:x1].max(axis=(1, 2))
    return y


def roi_pool_maxpool64(feat, rois, PH, scale, rule, k, stride, pad):
    """the two-step sequence: ROI pooling, then a floor-mode max-pool of the pooled maps"""
    return maxpool64(roi_pool64(feat, rois, PH, PH, scale, rule), k, stride, pad, 0)


def global_avg64(x):
    """mean over each map: [N, C, H, W] -> float64 [N, C]"""
    return np.asarray(x, np.float64).mean(axis=(2, 3))


def global_avg_seq32(x):
    """fp32 adds from 0 in row-major order, * float32(1 / (H * W))"""
    x = np.asarray(x, np.float32)
    N, C, H, W = x.shape
    acc = np.zeros((N, C), np.float32)
    for v in np.moveaxis(x.reshape(N, C, H * W), 2, 0):
        acc = acc + v
    return acc * (np.float32(1.0) / np.float32(H * W))


def bf16_round(a):
    """fp32 -> bf16 (round to nearest even) -> fp32; NaN and inf kept"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def value_class(a):
    """0 finite, 1 +inf, 2 -inf, 3 NaN"""
    a = np.asarray(a, np.float64)
    return np.where(np.isnan(a), 3, np.where(a == np.inf, 1, np.where(a == -np.inf, 2, 0)))


def mixed_sign(rng, shape, lo_exp=-6, hi_exp=6):
    """mixed-sign values whose magnitudes span 2^lo_exp .. 2^hi_exp (a range of at least 2^12)"""
    return (rng.choice([-1.0, 1.0], shape) * np.exp2(rng.uniform(lo_exp, hi_exp, shape))).astype(np.float32)


def roi_table(rng, n, H, W, scale):
    """n ROI rows (1, x1, y1, x2, y2) in image coordinates for an H x W map at `scale`: inside the map, across each border, wholly
    outside, inverted, one pixel, larger than the image — cycled, then jittered"""
    iw, ih = W / scale, H / scale
    base = [
        (0.25 * iw, 0.25 * ih, 0.75 * iw, 0.75 * ih),          # inside
        (-0.3 * iw, 0.2 * ih, 0.4 * iw, 0.8 * ih),             # across the left border
        (0.6 * iw, 0.1 * ih, 1.4 * iw, 0.7 * ih),              # right
        (0.2 * iw, -0.5 * ih, 0.9 * iw, 0.3 * ih),             # top
        (0.1 * iw, 0.6 * ih, 0.8 * iw, 1.6 * ih),              # bottom
        (1.5 * iw + 40, 0.2 * ih, 2.5 * iw + 80, 0.9 * ih),    # wholly outside (right)
        (0.1 * iw, -3.0 * ih - 80, 0.9 * iw, -1.5 * ih - 40),  # wholly outside (above)
        (0.8 * iw, 0.7 * ih, 0.3 * iw, 0.2 * ih),              # inverted
        (0.5 * iw, 0.5 * ih, 0.5 * iw, 0.5 * ih),              # one pixel
        (-0.5 * iw - 20, -0.5 * ih - 20, 1.5 * iw + 20, 1.5 * ih + 20),  # larger than the image
        (1.0, 1.0, iw, ih),                                    # the whole image
    ]
    rows = []
    for i in range(n):
        b = np.array(base[i % len(base)])
        if i >= len(base):
            b = b + rng.uniform(-0.2, 0.2, 4) * np.array([iw, ih, iw, ih])
        rows.append([1.0] + list(np.round(b + 1.0, 2)))
    return np.array(rows, np.float32)
