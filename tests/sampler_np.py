"""The minibatch sampler restated for the tests (test infrastructure; include/mpn.h mpn_attach_proposals / mpn_sample_rois, DESIGN.md
section 13.11): attach_proposals_kernel and roi_sample_kernel in numpy, fp32 in the stated operation order, the draws from
tests/dropout_np.py's Philox4x32-10 — and the inputs the CPU and the GPU tests share.

Every fp32 operation below is one numpy operation on float32 arrays, so each is rounded on its own, as the kernels' are
(-ffp-contract=off)."""
import numpy as np

import dropout_np as D

F1 = np.float32(1)
MASK32 = 0xFFFFFFFF


def _clip_wh(a, b):
    """the reference's clipping (utils.lua:106-116): x1 = a.x1, raised to b.x1 where smaller, ...; w = x2 - x1 + 1, h = y2 - y1 + 1"""
    a = np.asarray(a, np.float32).reshape(-1, 4)
    b = np.asarray(b, np.float32).reshape(4)
    x1, y1 = np.where(a[:, 0] < b[0], b[0], a[:, 0]), np.where(a[:, 1] < b[1], b[1], a[:, 1])
    x2, y2 = np.where(a[:, 2] > b[2], b[2], a[:, 2]), np.where(a[:, 3] > b[3], b[3], a[:, 3])
    w, h = (x2 - x1) + F1, (y2 - y1) + F1
    aarea = ((a[:, 2] - a[:, 0]) + F1) * ((a[:, 3] - a[:, 1]) + F1)
    return w.astype(np.float32), h.astype(np.float32), aarea.astype(np.float32)


def boxoverlap(a, b):
    """utils.boxoverlap in fp32: inter / ((aarea + barea) - inter), 0 where w < 0 or h < 0 -> (o, w, h)"""
    w, h, aarea = _clip_wh(a, b)
    b = np.asarray(b, np.float32).reshape(4)
    inter = w * h
    barea = ((b[2] - b[0]) + F1) * ((b[3] - b[1]) + F1)
    with np.errstate(divide="ignore", invalid="ignore"):
        o = inter / ((aarea + barea) - inter)
    o = np.where((w < 0) | (h < 0), np.float32(0), o)
    return o.astype(np.float32), w, h


def intersection(a, b):
    """utils.intersection in fp32: inter / aarea, NOT zeroed where w < 0 or h < 0 -> (ratio, w, h)"""
    w, h, aarea = _clip_wh(a, b)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (w * h) / aarea
    return r.astype(np.float32), w, h


def attach(proposals, gt, gt_labels, crowds=None):
    """attach_proposals_kernel: rows [gt ; proposals]; the loop over the GT boxes in order with a strict >, as the kernel runs it.
    -> dict boxes [m,4] f32, overlap [m] f32, overlap_raw (before the crowd mask), corr [m] i32, label [m] i32, crowd_max [m] f32"""
    prop = np.asarray(proposals, np.float32).reshape(-1, 4)
    gt = np.asarray(gt, np.float32).reshape(-1, 4)
    gl = np.asarray(gt_labels, np.int32).reshape(-1)
    crowds = np.zeros((0, 4), np.float32) if crowds is None else np.asarray(crowds, np.float32).reshape(-1, 4)
    g, m = gt.shape[0], gt.shape[0] + prop.shape[0]
    boxes = np.concatenate([gt, prop], 0)
    best, corr, label = np.zeros(m, np.float32), np.zeros(m, np.int32), np.zeros(m, np.int32)
    for j in range(g):
        o, _, _ = boxoverlap(boxes, gt[j])
        upd = np.ones(m, bool) if j == 0 else o > best
        best, corr, label = np.where(upd, o, best), np.where(upd, j + 1, corr).astype(np.int32), np.where(upd, gl[j], label).astype(np.int32)
    zero = best == 0
    corr[zero], label[zero] = 0, 0
    cmax = np.zeros(m, np.float32)
    for j in range(crowds.shape[0]):
        r, _, _ = intersection(boxes, crowds[j])
        cmax = r if j == 0 else np.where(r > cmax, r, cmax)
    mask = (cmax > np.float32(0.7)) & (np.arange(m) >= g) if crowds.shape[0] else np.zeros(m, bool)
    overlap = np.where(mask, np.float32(-1), best).astype(np.float32)
    return {"boxes": boxes, "overlap": overlap, "overlap_raw": best.astype(np.float32), "corr": corr, "label": label, "crowd_max": cmax.astype(np.float32)}


def crowd_mask_reference(boxes, crowds, g):
    """DataSetJSON.lua:345-363 transcribed line by line (float64 plays no part: the tensors are FloatTensors): inters [#crowds, m],
    maxinters = inters:max(1), mask = maxinters:gt(0.7), mask:narrow(1, 1, num_gt_boxes):fill(0)"""
    boxes = np.asarray(boxes, np.float32)
    inters = np.zeros((len(crowds), boxes.shape[0]), np.float32)
    for i, v in enumerate(crowds):
        inters[i] = intersection(boxes, v)[0]
    maxinters = inters.max(0)
    mask = maxinters > np.float32(0.7)
    mask[:g] = False
    return mask


def draw_words(seed, draw, s, r):
    """word 0 of Philox4x32-10(counter = (i, draw_lo, 0x80000000 + s, draw_hi), key = (seed_lo, seed_hi)) for i < r -> [r] uint32"""
    seed, draw = int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFFFFFFFFFF
    ctr = np.zeros((r, 4), np.uint64)
    ctr[:, 0] = np.arange(r, dtype=np.uint64)
    ctr[:, 1] = draw & MASK32
    ctr[:, 2] = 0x80000000 + int(s)
    ctr[:, 3] = draw >> 32
    return D.philox4x32_10(ctr, np.array([seed & MASK32, seed >> 32], np.uint64))[:, 0]


def index_map(words, count):
    """(uint64(word) * count) >> 32"""
    return ((np.asarray(words, np.uint64) * np.uint64(count)) >> np.uint64(32)).astype(np.int64)


def flip_boxes(b, width):
    """utils.flipBoxes in fp32: x1' = ((-x2) + W) + 1, x2' = ((-x1) + W) + 1"""
    b = np.asarray(b, np.float32).reshape(-1, 4)
    W = np.float32(width)
    out = b.copy()
    out[:, 0] = ((-b[:, 2]) + W) + F1
    out[:, 2] = ((-b[:, 0]) + W) + F1
    return out


def quotas(batch_size, fg_fraction):
    fg_num = int(float(fg_fraction) * int(batch_size))
    return int(batch_size) - fg_num, fg_num


def sample(rec, batch_size, fg_fraction, fg_thr, bg_lo, bg_hi, seed, draw, flip_width=0):
    """roi_sample_kernel -> dict rois [r,4], gt [r,4], labels [r], counts (n_bg, n_fg), rows [r] (the record rows drawn), r_bg, r_fg,
    bg / fg (the two lists)"""
    ov = rec["overlap"]
    fg = np.nonzero(ov >= np.float32(fg_thr))[0]
    bg = np.nonzero((ov >= np.float32(bg_lo)) & (ov < np.float32(bg_hi)))[0]
    bg_num, fg_num = quotas(batch_size, fg_fraction)
    r_bg, r_fg = min(bg_num, len(bg)), min(fg_num, len(fg))
    pick_bg = bg[index_map(draw_words(seed, draw, 0, r_bg), len(bg))] if r_bg else bg[:0]
    pick_fg = fg[index_map(draw_words(seed, draw, 1, r_fg), len(fg))] if r_fg else fg[:0]
    boxes, corr = rec["boxes"], rec["corr"]
    gt_fg = np.zeros((r_fg, 4), np.float32)
    has = corr[pick_fg] > 0
    gt_fg[has] = boxes[corr[pick_fg][has] - 1]
    rois = np.concatenate([boxes[pick_bg], boxes[pick_fg]], 0).astype(np.float32).reshape(-1, 4)
    gt = np.concatenate([np.zeros((r_bg, 4), np.float32), gt_fg], 0)
    labels = np.concatenate([np.zeros(r_bg, np.int32), rec["label"][pick_fg]]).astype(np.int32)
    if flip_width > 0:
        rois, gt = flip_boxes(rois, flip_width), flip_boxes(gt, flip_width)
    return {"rois": rois, "gt": gt, "labels": labels, "counts": (len(bg), len(fg)), "rows": np.concatenate([pick_bg, pick_fg]),
            "r_bg": r_bg, "r_fg": r_fg, "bg": bg, "fg": fg}


# ---------------------------------------------------------------------------------------------------------------------------------
# The shared inputs.  Ordinary boxes live in x <= 400, y <= 300.  G0 sits apart at (500..540, 500..560); the special proposals refer to it
# whether or not it is among the GT boxes.  Crowd 0 is a tall strip (every ordinary box has h > 0 against it, so the un-zeroed
# both-negative product cannot reach them), crowd 1 a wide strip that holds G0; further crowds are tall strips further right.
# ---------------------------------------------------------------------------------------------------------------------------------
G0 = np.array([500, 500, 540, 560], np.float32)
CROWD0 = np.array([600, 0, 650, 1000], np.float32)
CROWD1 = np.array([0, 495, 1000, 565], np.float32)
SPECIAL = np.array([
    [1000, 700, 1010, 710],    # 0 disjoint from every GT box: corr 0, label 0
    [541, 500, 560, 560],      # 1 touches G0: w == 0, overlap 0
    [545, 500, 570, 560],      # 2 right of G0: w = -4 < 0, h > 0 -> zeroed
    [700, 1100, 701, 1101],    # 3 off crowd 0's corner: w = -49, h = -99, inter = 4851 > 0, / aarea 4 -> masked although disjoint
    [600, 0, 650, 1000],       # 4 identical to crowd 0: masked
], np.float32)
N_CLASSES = 7


def make_case(n, g, n_crowd, seed=0):
    """-> (proposals [n,4], gt [g,4], gt_labels [g], crowds [n_crowd,4]).  GT 0 is G0, GT 1 its duplicate (the first index must win);
    the proposals start with SPECIAL (cut to n), then alternate jittered copies of GT boxes (foreground) and copies shifted by 0.45 of
    the width (background, IoU about 0.38)."""
    rng = np.random.default_rng(1000003 * n + 7919 * g + 104729 * n_crowd + seed)
    gt = np.zeros((g, 4), np.float32)
    for j in range(g):
        if j < 2:
            gt[j] = G0
        else:
            x1, y1 = rng.integers(20, 321), rng.integers(20, 221)
            gt[j] = [x1, y1, x1 + rng.integers(20, 81), y1 + rng.integers(20, 81)]
    gl = rng.integers(1, N_CLASSES, g).astype(np.int32)
    prop = np.zeros((n, 4), np.float32)
    k = min(n, len(SPECIAL))
    prop[:k] = SPECIAL[:k]
    for i in range(k, n):
        if g:
            b = gt[(i * 7) % g]
            if i % 2:
                prop[i] = b + rng.uniform(-3, 3, 4).astype(np.float32)
            else:
                prop[i] = b + np.float32(0.45) * (b[2] - b[0]) * np.array([1, 0, 1, 0], np.float32) + rng.uniform(-1, 1, 4).astype(np.float32)
        else:
            x1, y1 = rng.uniform(20, 320), rng.uniform(20, 220)
            prop[i] = [x1, y1, x1 + rng.uniform(20, 80), y1 + rng.uniform(20, 80)]
    crowds = np.zeros((n_crowd, 4), np.float32)
    for j in range(n_crowd):
        crowds[j] = CROWD0 if j == 0 else CROWD1 if j == 1 else [800 + 5 * j, 0, 803 + 5 * j, 1000]
    return prop, gt, gl, crowds


ATTACH_N = [0, 1, 63, 64, 65, 1000, 2049]
ATTACH_G = [0, 1, 3, 65]
ATTACH_CROWD = [0, 2, 65]


def attach_cases():
    """every (n, g, n_crowd) of the three lists with g + n > 0"""
    return [(n, g, c) for n in ATTACH_N for g in ATTACH_G for c in ATTACH_CROWD if n + g > 0]


# sampler cases: name -> (n, g, n_crowd, batch_size, fg_fraction, fg_thr, bg_lo, bg_hi)
SAMPLE_CASES = {
    "m60_few_fg": (57, 3, 0, 128, 0.25, 0.5, 0.1, 0.5),       # m < 64; n_fg < fg_num = 32: fewer than batch_size rows
    "m68_many_fg": (65, 3, 0, 16, 0.25, 0.5, 0.1, 0.5),       # m crosses 64; n_fg > fg_num = 4
    "m1003": (1000, 3, 2, 128, 0.25, 0.5, 0.1, 0.5),          # m < 1024, crowds: rows at -1
    "m2114_crowds": (2049, 65, 65, 128, 0.25, 0.5, 0.1, 0.5),  # m crosses 1024 twice: three chunks of the block scan
    "m1065_integral": (1000, 65, 2, 64, 0.5, 0.7, 0.0, 0.7),   # an IntegralSampler threshold pair; bg_lo = 0 takes the overlap-0 rows
}


def exact_threshold_records():
    """The two records whose overlaps are exact: row 1 = [1,1,10,10] against GT [1,1,10,5] is 50 / 100 = 0.5, against GT [1,1,1,10] it is
    10 / 100 = fl(0.1).  The other proposals are shifted copies that give each record background and foreground rows of its own."""
    out = {}
    for name, gtb in (("half", [1, 1, 10, 5]), ("tenth", [1, 1, 1, 10])):
        gt = np.array([gtb], np.float32)
        prop = np.array([[1, 1, 10, 10], [3, 1, 12, 5], [4, 2, 13, 6], [1, 3, 1, 14], [1, 4, 2, 13]], np.float32)
        out[name] = attach(prop, gt, np.array([3], np.int32))
    return out
