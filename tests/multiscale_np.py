"""Multi-scale testing (include/mpn.h mpn_frcnn_set_scales / mpn_project_im_rois_levels) restated in numpy
float32: getImages' level scales and sizes and the canvas (rules 1-2), the level of a ROI and its projected row (rules 3-4).
Test infrastructure; the device results are compared with np.array_equal where the contract says bit for bit."""
import math

import numpy as np

F32 = np.float32
TARGET_AREA = F32(224 * 224)


def c_round(x):
    """C round() of a non-negative double (half away from zero), as torch.round in ImageDetect.lua:36"""
    r = math.floor(x)
    return r + 1 if x - r >= 0.5 else r


def pick_scale(H, W, target, max_size):
    """ImageDetect.lua:34-38 in doubles (mpn_pick_scale)"""
    mn, mx = float(min(H, W)), float(max(H, W))
    s = target / mn
    if c_round(s * mx) > max_size:
        s = max_size / mx
    return s


def level_scales(H0, W0, targets, max_size):
    return [pick_scale(H0, W0, float(t), float(max_size)) for t in targets]


def level_size(H0, W0, s):
    """(H_l, W_l) = ((int)(H0*s), (int)(W0*s)); s == 1 keeps the image as it is"""
    return (H0, W0) if s == 1.0 else (int(H0 * s), int(W0 * s))


def canvas(H0, W0, scales):
    sizes = [level_size(H0, W0, s) for s in scales]
    return max(h for h, _ in sizes), max(w for _, w in sizes)


def distinct_levels(scales):
    """the levels a ROI can pick: the first of every run of equal scales"""
    return [l for l, s in enumerate(scales) if s not in scales[:l]]


def levels(boxes, scales):
    """rule 3: w = x2-x1+1, h = y2-y1+1, area = w*h, d_l = |area * (s_l*s_l) - 224^2|, every operation rounded to fp32; the level is
    THTensor_(min)'s index: start from d_0, take d_l when !(d_l >= min), stop once a NaN is taken."""
    b = np.asarray(boxes, F32).reshape(-1, 4)
    s = np.asarray(scales, np.float64).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        w = (b[:, 2] - b[:, 0]) + F32(1)
        h = (b[:, 3] - b[:, 1]) + F32(1)
        area = w * h
        d = np.abs(area[:, None] * (s * s)[None, :] - TARGET_AREA)
    out = np.zeros(b.shape[0], np.int64)
    for i in range(b.shape[0]):
        best, lvl = d[i, 0], 0
        for l in range(d.shape[1]):
            v = d[i, l]
            if not (v >= best):
                best, lvl = v, l
                if v != v:
                    break
        out[i] = lvl
    return out


def project(boxes, scales):
    """rule 4: rows {level + 1, (x1-1)*s_level+1, ...} in fp32 (project_rois_kernel's operation order); returns (rois [n,5], levels)"""
    b = np.asarray(boxes, F32).reshape(-1, 4)
    lv = levels(b, scales)
    s = np.asarray(scales, np.float64).astype(F32)[lv]
    rois = np.empty((b.shape[0], 5), F32)
    rois[:, 0] = (lv + 1).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        rois[:, 1:] = ((b + F32(-1)) * s[:, None]) + F32(1)
    return rois, lv
