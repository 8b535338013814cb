"""The layouts, orders and references of the conv-block half of multipathnet_amd/csrc/train.h, restated in NumPy for
tests/test_gpu_train_conv_kernels_numerics.py (test infrastructure).  Written from the header comments of
train.h, dense.h and mpn_internal.h: the C8P map with its halo, pitch padding and pad lanes; the `wpk` pack and the W' pack of the
Cout -> Cin convolution; the ordered ROI sum in both operand layouts; roi_bin_bounds' windows for both bin rules in fp32; the weight
gradient in float64 and the documented order of its segment sum; conv_bias_grad's order; the 2x2 ceil routing; the second stages of
the segmented forms; and the input sets of the GPU file, so that tests/test_train_conv_kernels_ref_cpu.py can show on the CPU that a plain
sequential fp32 evaluation of every one of them meets the bounds (tests/train_kernels_np.py derives the bound)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_kernels_np as R  # noqa: E402

F32, F64 = np.float32, np.float64
U23 = R.U23
SENT, SENT_F = R.SENT, R.SENT_F
SEG_PX, SEG_GROUP = 512, 8   # train.h kWgradSegPx, kWgradSegGroup
cdiv, round_up, bits, draw = R.cdiv, R.round_up, R.bits, R.draw
conv_pack, conv_unpack, conv_valid, conv_coutp, act_hp, act_wp = R.conv_pack, R.conv_unpack, R.conv_valid, R.conv_coutp, R.act_hp, R.act_wp


# ---- the C8P map -----------------------------------------------------------------------------------------------------------------------------
def c8p_pack(x, pad=0.0, halo=0.0, pitch=0.0):
    """[C, H, W] -> [Cb][Hp][Wp][8], Hp = 16 ceil(H / 16) + 2, Wp = 32 ceil(W / 32) + 2: pixel (y, x) of channel c at
    ((c / 8 * Hp + y + 1) * Wp + x + 1) * 8 + c % 8.  `halo`: the one-cell frame around the interior (rows 0 and H + 1, columns 0 and W + 1
    of the (H + 2) x (W + 2) corner); `pitch`: every other record outside the interior; `pad`: the channels >= C of the interior."""
    x = np.asarray(x, F32)
    C, H, W = x.shape
    out = np.full((cdiv(C, 8), act_hp(H), act_wp(W), 8), pitch, F32)
    out[:, :H + 2, :W + 2, :] = halo
    out[:, 1:H + 1, 1:W + 1, :] = pad
    for c in range(C):
        out[c // 8, 1:H + 1, 1:W + 1, c % 8] = x[c]
    return out


def c8p_unpack(m, C, H, W):
    m = np.asarray(m)
    return np.stack([m[c // 8, 1:H + 1, 1:W + 1, c % 8] for c in range(C)])


def c8p_masks(C, H, W):
    """-> (interior lanes of real channels, interior lanes of pad channels, everything outside the interior), three bool arrays"""
    shape = (cdiv(C, 8), act_hp(H), act_wp(W), 8)
    inner = np.zeros(shape, bool)
    inner[:, 1:H + 1, 1:W + 1, :] = True
    ch = (np.arange(shape[0])[:, None] * 8 + np.arange(8)[None, :]) < C
    real = inner & ch[:, None, None, :]
    return real, inner & ~real, ~inner


def dgrad_weights(w):
    """W'[ci][co][2 - ky][2 - kx] = W[co][ci][ky][kx] in Torch layout [Cin, Cout, 3, 3]: the weights of the Cout -> Cin convolution"""
    return np.ascontiguousarray(np.asarray(w).transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])


def dgrad_pack(w):
    """-> (wpk_t = the `wpk` pack of W' [Cout8 / 8][9][CinP][8] with pad lanes +0.0, zero_b [CinP])"""
    wt = dgrad_weights(w)
    return conv_pack(wt, 0.0), np.zeros(conv_coutp(wt.shape[0]), F32)


# ---- ROI pooling backward --------------------------------------------------------------------------------------------------------------------
def _roundf(v):
    """roundf on fp32 values: halves away from zero"""
    v = np.asarray(v, F64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def roi_windows(rois5, H, W, PH, PW, scale, rule):
    """roi_bin_bounds (coordinate offset 1, end_adjust 0) in fp32 -> hs, he [N, PH], ws, we [N, PW]: bin (ph, pw)'s window is
    [hs[ph], he[ph]) x [ws[pw], we[pw]).  rule 0: round the scaled corners, size >= 1, bins by the fp32 bin size, THEN clip; rule 1: round
    (x - 1) * scale + 1, minus 1, clip to the map FIRST, bins by integer products over the clipped crop."""
    r = np.asarray(rois5, F32)
    s, one = F32(scale), F32(1)
    out = []
    for lo, hi, size, P in ((r[:, 2], r[:, 4], H, PH), (r[:, 1], r[:, 3], W, PW)):
        p = np.arange(P, dtype=np.int64)[None, :]
        if rule == 0:
            a, b = _roundf((lo - one) * s), _roundf((hi - one) * s)
            n = np.maximum(b - a + 1, 1)
            bs = (n.astype(F32) / F32(P))[:, None]
            st = np.floor(p.astype(F32) * bs).astype(np.int64) + a[:, None]
            en = np.ceil((p + 1).astype(F32) * bs).astype(np.int64) + a[:, None]
            st, en = np.clip(st, 0, size), np.clip(en, 0, size)
        else:
            a, b = _roundf((lo - one) * s + one) - 1, _roundf((hi - one) * s + one) - 1
            a, b = np.clip(a, 0, size - 1), np.clip(b, 0, size - 1)
            n = np.maximum(b - a + 1, 1)[:, None]
            st = np.floor((p * n).astype(F32) / F32(P)).astype(np.int64) + a[:, None]
            en = np.ceil(((p + 1) * n).astype(F32) / F32(P)).astype(np.int64) + a[:, None]
        out += [st, en]
    return tuple(out)


def window_argmax(fmap, rois5, PH, PW, scale, rule):
    """the forward's arg-max [N, C, PH * PW] int32: first strict maximum from -inf in row-major scan of the bin's window, -1 for an empty
    window (or one that holds nothing above -inf)"""
    fmap = np.asarray(fmap, F32)
    C, H, W = fmap.shape
    hs, he, ws, we = roi_windows(rois5, H, W, PH, PW, scale, rule)
    out = -np.ones((len(rois5), C, PH * PW), np.int32)
    for n in range(len(rois5)):
        for ph in range(PH):
            for pw in range(PW):
                y0, y1, x0, x1 = hs[n, ph], he[n, ph], ws[n, pw], we[n, pw]
                if y1 <= y0 or x1 <= x0:
                    continue
                sub = fmap[:, y0:y1, x0:x1].reshape(C, -1)
                k = sub.argmax(1)
                idx = (y0 + k // (x1 - x0)) * W + x0 + k % (x1 - x0)
                out[n, :, ph * PW + pw] = np.where(sub.max(1) > -np.inf, idx, -1)
    return out


def argmax_in_windows(argmax, rois5, H, W, PH, PW, scale, rule):
    """every non-negative arg-max lies inside its bin's window: the condition under which the windowed sum equals the plain one"""
    hs, he, ws, we = roi_windows(rois5, H, W, PH, PW, scale, rule)
    am = np.asarray(argmax).reshape(len(rois5), -1, PH, PW)
    y, x = am // W, am % W
    ok = (y >= hs[:, None, :, None]) & (y < he[:, None, :, None]) & (x >= ws[:, None, None, :]) & (x < we[:, None, None, :])
    return bool((ok | (am < 0)).all())


def roi_rows_map(rois5, B):
    """by_batch: row n belongs to map clamp((int)rois[n][0] - 1, 0, B - 1) (the C cast truncates towards zero)"""
    return np.clip(np.trunc(np.asarray(rois5, F64)[:, 0]).astype(np.int64) - 1, 0, B - 1)


def roi_backward(g, argmax, rois5, by_batch, n0, n1, B, C, H, W, dtype=F32):
    """train.h's ordered sum: out[b][c][cell] = sum over the rows n in [n0, n1) of map b ascending, inside a row the bins ascending, of
    g[n][c][bin] where argmax[n][c][bin] == cell, added in `dtype` from +0.0.  g, argmax [N, C, PP] -> [B, C, H, W]"""
    g, am = np.asarray(g), np.asarray(argmax)
    N, _, PP = am.shape
    rows = roi_rows_map(rois5, B) if by_batch else np.zeros(N, np.int64)
    out = np.zeros((B, C, H * W), dtype)
    cs = np.arange(C)
    for n in range(n0, n1):
        o = out[rows[n]]
        for k in range(PP):
            i = am[n, :, k]
            ok = i >= 0
            o[cs[ok], i[ok]] = o[cs[ok], i[ok]] + g[n, ok, k].astype(dtype)   # one term per channel: no index repeats
    return out.reshape(B, C, H, W)


def roi_g_c8(g, Mp, fill=0.0, row_fill=None, rows=None):
    """g [N, C, PP] -> train_conv_backward's C8 matrix [Cb * PP][Mp][8]: g[n][c][bin] at record (c / 8) * PP + bin, row n, lane c % 8.
    Lanes c >= C and rows >= N hold `fill`; rows outside `rows` = (n0, n1) hold `row_fill`."""
    g = np.asarray(g, F32)
    N, C, PP = g.shape
    out = np.full((cdiv(C, 8) * PP, Mp, 8), fill, F32)
    for c in range(C):
        out[(c // 8) * PP:(c // 8 + 1) * PP, :N, c % 8] = g[:, c, :].T
    if rows is not None:
        out[:, :rows[0]] = row_fill
        out[:, rows[1]:N] = row_fill
    return out


# ---- the 3x3 convolution's weight and bias gradients -----------------------------------------------------------------------------------------
def _patches(x):
    """x [Cin, H, W] -> [9, Cin, H * W]: tap ky * 3 + kx holds X[ci][y + ky - 1][x + kx - 1], zero outside the map (the padding)"""
    Cin, H, W = x.shape
    xp = np.zeros((Cin, H + 2, W + 2), x.dtype)
    xp[:, 1:H + 1, 1:W + 1] = x
    return np.stack([xp[:, ky:ky + H, kx:kx + W].reshape(Cin, -1) for ky in range(3) for kx in range(3)])


def n_segments(H, W):
    return cdiv(H * W, SEG_PX)


def wgrad_slabs64(x, g):
    """float64: slab s = sum over the pixels [512 s, 512 (s + 1)) of the row-major map of G[co][p] * X[ci][p shifted by the tap]
    -> (slabs [nseg, Cout, Cin, 3, 3], the same sums of |G| |X|, the pixels per segment)"""
    x, g = np.asarray(x, F64), np.asarray(g, F64)
    Cout, H, W = g.shape
    P, A = _patches(x), _patches(np.abs(x))
    gf = g.reshape(Cout, -1)
    slabs, mags, npx = [], [], []
    for p0 in range(0, H * W, SEG_PX):
        p1 = min(p0 + SEG_PX, H * W)
        slabs.append(np.einsum("op,tip->oit", gf[:, p0:p1], P[:, :, p0:p1]))
        mags.append(np.einsum("op,tip->oit", np.abs(gf[:, p0:p1]), A[:, :, p0:p1]))
        npx.append(p1 - p0)
    shape = (len(npx), Cout, x.shape[0], 3, 3)
    return np.array(slabs).reshape(shape), np.array(mags).reshape(shape), npx


def wgrad_slabs_seq_f32(x, g):
    """the same slabs by a plain fp32 chain over the segment's pixels ascending, product and sum rounded separately"""
    x, g = np.asarray(x, F32), np.asarray(g, F32)
    Cout, H, W = g.shape
    P = np.ascontiguousarray(_patches(x).transpose(2, 1, 0))   # [pixel, Cin, 9]
    gf = np.ascontiguousarray(g.reshape(Cout, -1).T)           # [pixel, Cout]
    slabs = []
    for p0 in range(0, H * W, SEG_PX):
        acc = np.zeros((Cout, x.shape[0], 9), F32)
        for p in range(p0, min(p0 + SEG_PX, H * W)):
            acc = acc + gf[p][:, None, None] * P[p][None]
        slabs.append(acc)
    return np.array(slabs).reshape(len(slabs), Cout, x.shape[0], 3, 3)


def group_sum_f32(slabs):
    """the documented second stage on slabs [nseg, ...]: each group of SEG_GROUP consecutive slabs added ascending from +0.0, the group
    sums added ascending (the first taken as it is); up to SEG_GROUP slabs it is the plain ascending sum"""
    slabs = np.asarray(slabs, F32)
    v = None
    for g0 in range(0, slabs.shape[0], SEG_GROUP):
        gs = np.zeros(slabs.shape[1:], F32)
        for s in range(g0, min(g0 + SEG_GROUP, slabs.shape[0])):
            gs = gs + slabs[s]
        v = gs if v is None else v + gs
    return v


def wgrad_reduce_f32(part, Cin, Cout, dw_old=None):
    """conv3x3_wgrad's dW from its own partial sums: part [nseg][Cin8 / 8][9][CoutP][8] -> the packed dW; lanes outside the layer +0.0
    whatever part and dw_old hold there; dw_old (accumulate): f32(dw_old + v)"""
    valid = conv_valid(Cin, Cout)
    with np.errstate(invalid="ignore"):
        v = group_sum_f32(part)
        if dw_old is not None:
            v = np.asarray(dw_old, F32) + v
    return np.where(valid, v, F32(0)).astype(F32)


def slabs_pack(slabs, fill=0.0):
    """[nseg, Cout, Cin, 3, 3] -> [nseg][Cin8 / 8][9][CoutP][8]"""
    return np.stack([conv_pack(s, fill) for s in slabs])


def slabs_unpack(part, Cin, Cout):
    return np.stack([conv_unpack(p, Cin, Cout) for p in part])


def bias_grad_f32(g, db_old=None):
    """conv_bias_grad's order on g [Cout, H, W]: slot s adds the pixels s, s + 32, ... of the row-major map ascending from +0.0, then the
    tree 16, 8, 4, 2, 1 (sgd_bias_kernel's order over pixels); db_old (accumulate): f32(db_old + sum)"""
    g = np.asarray(g, F32)
    s = R.bias_sum_f32(g.reshape(g.shape[0], -1).T)
    return s if db_old is None else np.asarray(db_old, F32) + s


# ---- the 2x2 ceil-mode pool's routing --------------------------------------------------------------------------------------------------------
def pool_backward(x, gy, relu_mask):
    """include/mpn.h mpn_maxpool2x2_ceil_backward: per window the scan from -inf with v > m over (2Y,2X), (2Y,2X+1), (2Y+1,2X),
    (2Y+1,2X+1), cells outside the map skipped; gy goes to the cell the scan ends on (relu_mask: only if that cell is > 0), +0.0 to
    every other cell.  A window of NaN and / or -inf cells routes nowhere."""
    x, gy = np.asarray(x, F32), np.asarray(gy, F32)
    C, H, W = x.shape
    dx = np.zeros((C, H, W), F32)
    for Y in range((H + 1) // 2):
        for X in range((W + 1) // 2):
            m = np.full(C, -np.inf, F32)
            win = -np.ones(C, np.int64)
            cells = [(2 * Y + dy, 2 * X + dx_) for dy in (0, 1) for dx_ in (0, 1)]
            for q, (yy, xx) in enumerate(cells):
                if yy < H and xx < W:
                    with np.errstate(invalid="ignore"):
                        take = x[:, yy, xx] > m
                    m, win = np.where(take, x[:, yy, xx], m), np.where(take, q, win)
            if relu_mask:
                win = np.where(m > 0, win, -1)
            for q, (yy, xx) in enumerate(cells):
                if yy < H and xx < W:
                    dx[:, yy, xx] = np.where(win == q, gy[:, Y, X], F32(0))
    return dx


# ---- the segmented forms' second stages ------------------------------------------------------------------------------------------------------
def seg_pack(a, Mp, chunks, lane_fill=0.0, row_fill=0.0):
    """[nseg, B, N] -> a C8 matrix at row pitch nseg * Mp: row seg * Mp + m; lanes >= N of valid rows `lane_fill`, every other row `row_fill`"""
    a = np.asarray(a, F32)
    nseg, B, N = a.shape
    out = np.full((chunks, nseg, Mp, 8), row_fill, F32)
    out[:, :, :B, :] = lane_fill
    for n in range(N):
        out[n // 8, :, :B, n % 8] = a[:, :, n]
    return out.reshape(chunks, nseg * Mp, 8)


def seg_x_pack(x, Mp, row_fill=0.0):
    """the operand of the packed weight (inner = 1): K64 / 8 chunks, pad k lanes of valid rows +0.0 (linear_c8's operand: read and discarded)"""
    return seg_pack(x, Mp, R.k64(x.shape[2]) // 8, 0.0, row_fill)


def seg_bias_f32(g):
    """sgd_bias_seg_c8's db on g [nseg, B, N]: per segment sgd_bias_kernel's sum; the segment sums in blocks of 64 leaves (missing: +0.0)
    through the tree 32, 16, ..., 1; the blocks' roots added ascending (the first taken as it is)"""
    g = np.asarray(g, F32)
    nseg, _, N = g.shape
    total = None
    for s0 in range(0, nseg, 64):
        leaves = np.zeros((64, N), F32)
        for s in range(s0, min(s0 + 64, nseg)):
            leaves[s - s0] = R.bias_sum_f32(g[s])
        w = 32
        while w:
            leaves[:w] = leaves[:w] + leaves[w:2 * w]
            w //= 2
        total = leaves[0].copy() if total is None else total + leaves[0]
    return total


# ---- input sets of the GPU file --------------------------------------------------------------------------------------------------------------
WGRAD_SHAPES = ((1, 1, 1, 1), (3, 7, 1, 2), (8, 8, 3, 3), (9, 33, 5, 7), (24, 129, 2, 9), (32, 32, 16, 32), (8, 40, 19, 27), (8, 8, 64, 64),
                (8, 8, 17, 241), (12, 20, 91, 91), (64, 16, 21, 34))   # (Cin, Cout, H, W)
BIAS_EXTRA = ((12, 1, 1), (12, 1, 31), (12, 4, 8), (12, 3, 11))        # (Cout, H, W): H * W = 1, 31, 32, 33


def wgrad_inputs(Cin, Cout, H, W, exact=False):
    """two images' (x [Cin, H, W], g [Cout, H, W]); exact: integers in [-2, 2], so every partial sum is an integer below 2^24"""
    rng = np.random.default_rng([Cin, Cout, H, W, int(exact), 21])
    if exact:
        return [(rng.integers(-2, 3, (Cin, H, W)).astype(F32), rng.integers(-2, 3, (Cout, H, W)).astype(F32)) for _ in range(2)]
    return [(draw(rng, (Cin, H, W)), draw(rng, (Cout, H, W))) for _ in range(2)]


def bias_maps():
    return [(Cout, H, W) for _, Cout, H, W in WGRAD_SHAPES] + list(BIAS_EXTRA)


def bias_inputs(Cout, H, W, exact=False):
    rng = np.random.default_rng([Cout, H, W, int(exact), 22])
    if exact:
        return [rng.integers(-2, 3, (Cout, H, W)).astype(F32) for _ in range(2)]
    return [draw(rng, (Cout, H, W)) for _ in range(2)]


# (C, H, W, PH, PW, N, by_batch B or 0 for the row-range form)
ROI_CASES = ((8, 5, 7, 7, 7, 24, 0), (1, 1, 1, 7, 7, 9, 0), (12, 21, 34, 7, 7, 37, 0), (40, 21, 34, 3, 5, 21, 0), (8, 21, 34, 32, 32, 6, 0),
             (12, 5, 7, 1, 1, 24, 0), (8, 5, 7, 7, 7, 24, 1), (12, 21, 34, 7, 7, 37, 3), (40, 5, 7, 3, 5, 21, 3), (1, 21, 34, 32, 32, 6, 1))
ROI_SCALE = 0.25


def roi_inputs(C, H, W, PH, PW, N, B):
    """-> (feature maps [max(B, 1), C, H, W], rois [N, 5], g [N, C, PP]).  Beside random boxes: corners whose projection (x - 1) * scale
    is exactly k + 0.5 and -(k + 0.5), x2 < x1, a box wholly outside, the whole map, duplicates; by_batch: batch indices 0, B + 2 and -3."""
    rng = np.random.default_rng([C, H, W, PH, PW, N, B, 23])
    nb = max(B, 1)
    feat = draw(rng, (nb, C, H, W), zero_frac=0.05)
    s = 1.0 / ROI_SCALE
    c = rng.uniform([-8, -8], [s * W + 8, s * H + 8], (N, 2))
    wh = rng.uniform(4, max(8.0, 3.0 * max(H, W)), (N, 2))
    rois = np.concatenate([rng.integers(1, nb + 1, (N, 1)), c - wh / 2, c + wh / 2], 1).astype(F32)
    half = lambda k: 1.0 + s * (k + 0.5)   # (x - 1) * scale == k + 0.5 exactly: s is a power of two
    special = [
        [1, half(0), half(1), half(2), half(3)], [1, half(-1), half(-2), half(1), half(0)], [1, half(-3), half(-1), half(-1), half(2)],
        [1, half(2), half(1), half(0), half(0)],                                  # x2 < x1, y2 < y1
        [1, s * W + 40, s * H + 40, s * W + 60, s * H + 60],                      # wholly outside
        [1, 1, 1, 1 + s * (W - 1), 1 + s * (H - 1)],                              # the whole map
        [1, half(W - 2), half(H - 2), half(W - 1), half(H - 1)],                  # half-integer corners at the far border
    ]
    for i, row in enumerate(special):
        if 2 * i + 1 < N:
            rois[2 * i + 1, 1:] = row[1:]
    if N > 16:
        rois[16], rois[0] = rois[3], rois[3]   # duplicates: several rows add into the same cells
    if B:
        rois[2 % N, 0], rois[4 % N, 0], rois[6 % N, 0] = 0, B + 2, -3
    g = draw(rng, (N, C, PH * PW))
    return feat, rois, g


def roi_row_ranges(N):
    """(n0, n1) of the row-range form: all rows, n0 > 0, n1 < N, both, and the empty range"""
    return sorted({(0, N), (min(3, N - 1), N), (0, N - 2), (N // 3, N - N // 4), (N // 2, N // 2)})


ROI_SYNTH_CASES = ((33, 2, 1, 1), (2, 33, 12, 3), (7, 7, 12, 3))   # (PH, PW, C, B)
ROI_SYNTH_MAP = (5, 7, 11)                                          # H, W, N


def roi_synth_inputs(PH, PW, C, B):
    """arg-max values no forward produced: any cell or -1, and every third bin of every row into one of three cells -> (argmax, g, rois)"""
    H, W, N = ROI_SYNTH_MAP
    rng = np.random.default_rng([PH, PW, C, B])
    am = rng.integers(-1, H * W, (N, C, PH * PW)).astype(np.int32)
    am[:, :, ::3] = rng.integers(0, 3, (N, C, 1))   # many rows and bins add into the same three cells
    g = draw(rng, (N, C, PH * PW))
    rois = np.concatenate([rng.integers(-1, B + 3, (N, 1)), rng.uniform(1, 20, (N, 4))], 1).astype(F32)
    return am, g, rois


POOL_SHAPES = ((1, 1, 1), (3, 1, 5), (8, 2, 2), (12, 7, 9), (40, 21, 34))


def pool_inputs(C, H, W):
    """x [C, H, W] post-ReLU-like with negative values too, and windows with ties, all <= 0, -0.0, NaN cells, all NaN, all -inf"""
    rng = np.random.default_rng([C, H, W, 24])
    x = draw(rng, (C, H, W), zero_frac=0.2)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    kind = rng.integers(0, 10, (C, Ho, Wo))
    flat = kind.reshape(-1)
    flat[:min(8, flat.size)] = np.arange(min(8, flat.size))   # every kind is present wherever the map has room
    for c in range(C):
        for Y in range(Ho):
            for X in range(Wo):
                sl = (c, slice(2 * Y, 2 * Y + 2), slice(2 * X, 2 * X + 2))
                k = kind[c, Y, X]
                if k == 0:
                    x[sl] = F32(1.5)            # a tie: the first cell in scan order wins
                elif k == 1:
                    x[sl] = -np.abs(x[sl])      # all <= 0
                elif k == 2:
                    x[sl] = F32(-0.0)
                elif k == 3:
                    x[c, 2 * Y, 2 * X] = np.nan  # a NaN cell never wins
                elif k == 4:
                    x[sl] = np.nan
                elif k == 5:
                    x[sl] = -np.inf
                elif k == 6:
                    x[sl] = F32(0.0)
                    x[c, min(2 * Y + 1, H - 1), min(2 * X + 1, W - 1)] = F32(2.0 ** -126)
    gy = draw(rng, (C, Ho, Wo), zero_frac=0.0)
    return x, gy


# (nseg, N, K, B, Mp): every value of every parameter; nseg 9, 65 and 130 with N % 8 != 0
SEG_CASES = ((1, 1, 8, 1, 128), (8, 7, 100, 2, 128), (9, 7, 112, 3, 128), (49, 48, 112, 7, 128), (64, 48, 8, 8, 128), (65, 129, 264, 9, 128),
             (130, 7, 100, 70, 128), (9, 129, 8, 70, 256), (65, 1, 100, 3, 256), (49, 48, 264, 70, 256), (130, 129, 8, 1, 128))


def seg_inputs(nseg, N, K, B):
    rng = np.random.default_rng([nseg, N, K, B, 25])
    return draw(rng, (nseg, B, N)), draw(rng, (nseg, B, K))   # g, x


SCALE_N = (1, 2, 3, 4, 5, 7, 1023, 4099, 4 * 256 * 4096 + 1029)
SCALE_F = (0.0, 1.0, float(F32(0.1)), 2.0 ** -130)


def scale_inputs(n):
    """ordinary non-zero values with +-0, subnormals, +-inf, NaN and 2^-126 among them — but never in the last four floats, so that an
    element the scalar tail (or the last record) skipped cannot hide behind 0 * f = 0 or NaN * f = NaN"""
    rng = np.random.default_rng([n % 100003, 26])
    v = draw(rng, n, zero_frac=0.0)
    sp = np.array([0.0, -0.0, 2.0 ** -140, -(2.0 ** -149), np.inf, -np.inf, np.nan, 2.0 ** -126], F32)
    if n > 4:
        idx = rng.permutation(n - 4)[:min(n - 4, 64)]
        v[idx] = sp[np.arange(idx.size) % sp.size]
    return v


DGRAD_PACK_SHAPES = ((1, 1), (3, 7), (8, 16), (12, 20), (24, 129), (136, 32))   # (Cin, Cout)
SPLIT_CKK = ((2, 1), (7, 3), (81, 2))
SPLIT_B = (1, 129, 300)
