"""NumPy restatements of the layouts the data-movement kernels convert between, written from the formulas of multipathnet_amd/csrc/dense.h
(C8P, C8, the packed weights), graph_internal.h (C8I) and the comments above the kernels (mosaic, im2col rows, the shard and detection
records) as plain index loops — not from the kernels' thread arithmetic.  tests/test_layout_ref_cpu.py checks each one against an
independent torch formulation; tests/test_gpu_layout_kernels.py compares the kernels with them bit for bit.  The shape lists both modules
run are here too.  Where an older module already states a layout it is reused: train_conv_kernels_np.c8p_pack / c8p_unpack / c8p_masks,
train_kernels_np.c8_pack / c8_unpack / conv_pack / lin_pack, train_phase2_kernels_np.slab_pack / slab_unpack."""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_conv_kernels_np as K  # noqa: E402
import train_kernels_np as R  # noqa: E402
import train_phase2_kernels_np as Q  # noqa: E402

F32, F64 = np.float32, np.float64
SENT, SENT_F = R.SENT, R.SENT_F
cdiv, round_up, bits, draw = R.cdiv, R.round_up, R.bits, R.draw
act_hp, act_wp, conv_coutp = R.act_hp, R.act_wp, R.conv_coutp
c8p_pack, c8p_unpack, c8p_masks = K.c8p_pack, K.c8p_unpack, K.c8p_masks
c8_pack, c8_unpack, conv_pack, lin_pack = R.c8_pack, R.c8_unpack, R.conv_pack, R.lin_pack
pooled_pack, pooled_unpack = Q.slab_pack, Q.slab_unpack   # [N, C, PP] <-> [ceil(C / 8) * PP][Mp][8]

# ---- the shape lists ---------------------------------------------------------------------------------------------------------------------
MAP_HW = ((1, 1), (2, 3), (16, 32), (17, 33))        # act_hp steps at 16, act_wp at 32
MAP_C = (1, 3, 8, 9, 17)
ROWMAJOR_M, ROWMAJOR_K = (1, 127, 128, 129), (1, 7, 8, 9, 65)
CONV_CIN, CONV_COUT, FIRST_CIN = (3, 8, 9, 64), (1, 127, 128, 129), (1, 3, 4)
HALO_N = (1, 2, 24, 25, 49)                           # kHaloMax = 24: one, two and three launches
HALO_C, HALO_HW = (3, 8, 17), ((1, 1), (16, 32), (17, 33), (5, 40))
POOL_HW, POOL_C = ((1, 1), (2, 2), (3, 5), (16, 32), (17, 33)), (3, 8, 9)
SHARD_ROWS = ((1, 1, 1, 2), (5, 2, 1, 3), (7, 3, 2, 21), (3, 4, 1, 2))   # (N, world, P, C)
SHARD_CLS, SHARD_WORLD, SHARD_NROWS = (1, 5, 20), (1, 2, 3, 7), (1, 64, 257)
DET_CAP = (1, 100)
C8I_CB = (1, 3)
MOSAIC = ((1, 7, 7, 1), (5, 7, 7, 2), (6, 3, 4, 3))   # (N, H, W, mx)
MOSAIC_SPARE = 3                                      # the mosaic is laid out for N + 3 maps
IM2COL_K = ((3, 3, 1, 1), (7, 7, 2, 3), (11, 11, 4, 2))  # (KH, KW, stride, pad)
IM2COL_HW = ((11, 13), (23, 17))
PERMUTE_COUT, PERMUTE_KK = (1, 5, 64), (9, 49)
GCONV_KK, GCONV_CIN, GCONV_COUT = (1, 9, 49), (3, 8, 9), (1, 129)
IMAGE_SWAPS, IMAGE_SCALES = ((2, 1, 0), (0, 1, 2)), (1.0, 255.0)
CANVAS_EXTRA = ((0, 0), (1, 0), (0, 5))


def lin_mp(M):
    return round_up(M, 128)


def values(seed, shape):
    """the module's ordinary values: magnitudes in [2^-6, 2^3], both signs, exact zeros, and one each of -0.0, +-inf, a denormal and FLT_MAX"""
    rng = np.random.default_rng(seed)
    v = draw(rng, shape).reshape(-1)
    sp = np.array([-0.0, np.inf, -np.inf, 1e-42, -3.4028234663852886e38], F32)
    v[:min(v.size, sp.size)] = sp[:v.size]
    return rng.permutation(v).reshape(shape)


# ---- packed first-layer weights ----------------------------------------------------------------------------------------------------------
def conv_first_pack(w, fill=0.0):
    """[Cout, Cin <= 4, 3, 3] -> [36][CoutP]: row (tap * 2 + p) * 2 + half holds input channel 2 p + half of tap ky * 3 + kx"""
    w = np.asarray(w, F32)
    Cout, Cin = w.shape[:2]
    out = np.full((36, conv_coutp(Cout)), fill, F32)
    for tap in range(9):
        for p in range(2):
            for half in range(2):
                cin = 2 * p + half
                if cin < Cin:
                    out[(tap * 2 + p) * 2 + half, :Cout] = w[:, cin, tap // 3, tap % 3]
    return out


# ---- the graph executor's packed weights ---------------------------------------------------------------------------------------------------
def gconv_pack(w, nch=None, fill=0.0):
    """[Cout, Cin, KK] -> [KK][nch][CoutP][8]: lane j of chunk ch of tap t holds w[co, 8 ch + j, t]; nch = ceil(Cin / 8) unless given"""
    w = np.asarray(w, F32)
    Cout, Cin, KK = w.shape
    nch = cdiv(Cin, 8) if nch is None else nch
    out = np.full((KK, nch, round_up(Cout, 128), 8), fill, F32)
    for t in range(KK):
        for ci in range(Cin):
            out[t, ci // 8, :Cout, ci % 8] = w[:, ci, t]
    return out


def f2bf_bits(x):
    """fp32 -> bf16 bits (uint16), round to nearest even on the integer pattern: add 0x7FFF plus the kept part's last bit, keep the high half.
    (Finite values and infinities; a value above the largest bf16 becomes inf this way, as IEEE rounding wants.)"""
    u = bits(x).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def permute_w3(w):
    """[Cout, 3, KK] -> [Cout, KK * 3], k = tap * 3 + c"""
    w = np.asarray(w, F32)
    Cout, _, KK = w.shape
    out = np.empty((Cout, KK * 3), F32)
    for tap in range(KK):
        for c in range(3):
            out[:, tap * 3 + c] = w[:, c, tap]
    return out


# ---- the image transformer -----------------------------------------------------------------------------------------------------------------
def image_transform(img, swap, scale, mean, std, has_std):
    """[3, H, W] fp32 -> [3, H, W] fp32: float32(((double)v * scale + (-mean)) / std), the multiply only when scale != 1, the divide only
    with has_std; output channel j reads plane swap[j]"""
    img = np.asarray(img, F32)
    out = np.empty(img.shape, F32)
    for j in range(3):
        v = img[swap[j]].astype(F64)
        if scale != 1.0:
            v = v * F64(scale)
        v = v + (-F64(mean[j]))
        if has_std:
            v = v / F64(std[j])
        out[j] = v.astype(F32)
    return out


IMAGE_STD = (0.5, 2.0, 57.375)   # powers of two on the channels with special pixels: the division keeps a tie a tie


def image_case(H, W, swap, scale, seed):
    """-> (img [3, H, W], mean[3]).  Output channel 0: pixel 0 cancels to the denormal 2^-140.  Output channel 1: pixel 0 gives
    1 + 2^-23 + 2^-24 in double, a float rounding tie whose even neighbour is above; pixel 1 (if there is one) the tie one float further,
    whose even neighbour is below.  Output channel 2: an ordinary mean."""
    rng = np.random.default_rng([H, W, int(scale), seed])
    img = (rng.random((3, H, W)) * (255.0 / scale)).astype(F32)
    img[:, 0, 0] = 0.5
    img[swap[0], 0, 0] = F32(2.0 ** -120)   # (v * scale and the mean below are exact doubles some 2^-120 large, 2^-140 apart)
    mean = [0.0, 0.0, 102.9801]
    mean[0] = float(F64(img[swap[0], 0, 0]) * scale - 2.0 ** -140)
    mean[1] = float(F64(img[swap[1], 0, 0]) * scale - (1.0 + 2.0 ** -23 + 2.0 ** -24))
    if W > 1:
        img[swap[1], 0, 1] = F32(0.5 + 2.0 ** -23)
    return img, mean


def image_c8p(t, Hc, Wc, outside=0.0):
    """transformed [3, H, W] -> the one-block C8P map of an Hc x Wc canvas: the image top-left, every other interior lane +0.0 (channels
    3..7 included), halo and pitch padding `outside`"""
    _, H, W = t.shape
    out = np.full((1, act_hp(Hc), act_wp(Wc), 8), outside, F32)
    out[0, 1:Hc + 1, 1:Wc + 1, :] = 0
    for c in range(3):
        out[0, 1:H + 1, 1:W + 1, c] = t[c]
    return out


# ---- 2x2 / stride 2 ceil-mode max-pool -----------------------------------------------------------------------------------------------------
def maxpool2x2(x):
    """[C, H, W] -> [C, ceil(H / 2), ceil(W / 2)]: m = -inf, then `if v > m: m = v` over the window's pixels inside the map in row-major
    order: a NaN never wins, an all-NaN window gives -inf, and of +0.0 and -0.0 the first one met stays"""
    x = np.asarray(x, F32)
    C, H, W = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    out = np.full((C, Ho, Wo), -np.inf, F32)
    for y in range(Ho):
        for xx in range(Wo):
            m = out[:, y, xx]
            for dy in range(2):
                for dx in range(2):
                    if 2 * y + dy < H and 2 * xx + dx < W:
                        v = x[:, 2 * y + dy, 2 * xx + dx]
                        with np.errstate(invalid="ignore"):
                            m = np.where(v > m, v, m)
            out[:, y, xx] = m
    return out


def pool_input(C, H, W, seed):
    """values with windows of NaNs, one all-NaN window, -0.0 against +0.0 in both orders, and -inf"""
    x = values([C, H, W, seed], (C, H, W))
    flat = x.reshape(C, -1)
    n = flat.shape[1]
    flat[0, 0] = np.nan
    if H >= 2 and W >= 2:
        x[C - 1, 0:2, 0:2] = np.nan                       # an all-NaN window
        x[0, 0, 0], x[0, 0, 1], x[0, 1, 0], x[0, 1, 1] = -0.0, 0.0, -np.inf, np.nan
    if H >= 3 and W >= 4:
        x[0, 0, 2], x[0, 0, 3], x[0, 1, 2], x[0, 1, 3] = 0.0, -0.0, -np.inf, -np.inf
        x[0, 2:4, 0:2] = np.nan                            # a window of -inf and NaNs only (one row of it at H = 3)
        x[0, 2, 0] = -np.inf
    if n == 1 and C > 1:
        flat[1, 0] = -np.inf
    return x


# ---- the halo -----------------------------------------------------------------------------------------------------------------------------
def halo_records(H, W):
    """records per plane outside the interior, counted as c8p_zero_halos states it: whole rows 0 and H + 1 .. Hp - 1, then column 0 and
    columns W + 1 .. Wp - 1 of rows 1 .. H"""
    Hp, Wp = act_hp(H), act_wp(W)
    return Wp * (Hp - H) + H * (Wp - W)


def halo_mask(C, H, W):
    """bool [Cb][Hp][Wp][8]: everything of each plane outside the H x W interior"""
    m = np.ones((cdiv(C, 8), act_hp(H), act_wp(W), 8), bool)
    m[:, 1:H + 1, 1:W + 1, :] = False
    return m


def halo_list(n):
    """n (C, H, W) geometries cycling through HALO_C x HALO_HW, so that every list of two or more mixes geometries"""
    geo = list(itertools.product(HALO_HW, HALO_C))
    return [(geo[(5 * i) % len(geo)][1],) + geo[(5 * i) % len(geo)][0] for i in range(n)]


# ---- the shard partition ---------------------------------------------------------------------------------------------------------------------
def shard_bounds(n, world, rank):
    """balanced contiguous partition: the first n % world ranks own one item more -> [lo, hi)"""
    base, rem = n // world, n % world
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def shard_owner(item, n, world):
    """-> (rank, index inside the rank's range).  n < world: base = 0, every item is below the cut and no division by base is reached"""
    base, rem = n // world, n % world
    cut = rem * (base + 1)
    if item < cut:
        return item // (base + 1), item % (base + 1)
    q = (item - cut) // base
    return rem + q, item - cut - q * base


def shard_rows_record(sc, bb, N, world, rank, P, C):
    """this rank's tables sc [P, n_local, C], bb [P, n_local, 4C] -> [scores: P x chunk x C][boxes: P x chunk x 4C], rows at and beyond
    n_local +0.0"""
    chunk = cdiv(N, world)
    lo, hi = shard_bounds(N, world, rank)
    s, b = np.zeros((P, chunk, C), F32), np.zeros((P, chunk, 4 * C), F32)
    s[:, :hi - lo], b[:, :hi - lo] = sc, bb
    return np.concatenate([s.reshape(-1), b.reshape(-1)])


def shard_rows_join(all_rec, N, world, P, C):
    """[world][rec] -> (sc [P, N, C], bb [P, N, 4C]) in the unsharded row order"""
    chunk = cdiv(N, world)
    all_rec = np.asarray(all_rec).reshape(world, -1)
    sc, bb = np.empty((P, N, C), all_rec.dtype), np.empty((P, N, 4 * C), all_rec.dtype)
    for row in range(N):
        owner, i = shard_owner(row, N, world)
        s = all_rec[owner, :P * chunk * C].reshape(P, chunk, C)
        b = all_rec[owner, P * chunk * C:].reshape(P, chunk, 4 * C)
        sc[:, row], bb[:, row] = s[:, i], b[:, i]
    return sc, bb


def class_rec_floats(cmax, rows, voting):
    return cmax * (1 + rows * (11 if voting else 6))


def clamp_count(n, rows):
    return min(max(int(n), 0), rows)


def shard_class_record(keep, kidx, n_keep, voted, n_cls, world, rank, rows):
    """the class record of a rank as 32-bit words: [n_keep: cmax][keep: cmax x rows x 5][keep_idx: cmax x rows][voted: cmax x rows x 5 if
    voting]; slot j = class c0 + j, count clamped to 0..rows (0 for a slot past the rank's range), rows at and beyond the count SENT"""
    cmax = cdiv(n_cls, world)
    c0, c1 = shard_bounds(n_cls, world, rank)
    rec = np.full(class_rec_floats(cmax, rows, voted is not None), SENT, np.uint32)
    cnt = rec[:cmax]
    rk = rec[cmax:cmax + cmax * rows * 5].reshape(cmax, rows, 5)
    ri = rec[cmax + cmax * rows * 5:cmax + cmax * rows * 6].reshape(cmax, rows)
    rv = rec[cmax + cmax * rows * 6:].reshape(cmax, rows, 5) if voted is not None else None
    for j in range(cmax):
        c = c0 + j
        n = clamp_count(n_keep[c], rows) if c < c1 else 0
        cnt[j] = n
        if n == 0:
            continue
        rk[j, :n] = bits(keep[c, :n])
        ri[j, :n] = np.asarray(kidx[c, :n], np.int32).view(np.uint32)
        if rv is not None:
            rv[j, :n] = bits(voted[c, :n])
    return rec


def shard_class_join(all_rec, n_cls, world, rows, voting):
    """[world][rec] (uint32) -> (keep, kidx, n_keep, voted or None) as 32-bit words, rows at and beyond each count SENT"""
    cmax = cdiv(n_cls, world)
    all_rec = np.asarray(all_rec, np.uint32).reshape(world, -1)
    keep = np.full((n_cls, rows, 5), SENT, np.uint32)
    kidx = np.full((n_cls, rows), SENT, np.uint32)
    voted = np.full((n_cls, rows, 5), SENT, np.uint32) if voting else None
    n_keep = np.empty(n_cls, np.int32)
    for c in range(n_cls):
        owner, j = shard_owner(c, n_cls, world)
        rec = all_rec[owner]
        n = clamp_count(rec[:cmax].view(np.int32)[j], rows)
        n_keep[c] = n
        keep[c, :n] = rec[cmax:cmax + cmax * rows * 5].reshape(cmax, rows, 5)[j, :n]
        kidx[c, :n] = rec[cmax + cmax * rows * 5:cmax + cmax * rows * 6].reshape(cmax, rows)[j, :n]
        if voting:
            voted[c, :n] = rec[cmax + cmax * rows * 6:].reshape(cmax, rows, 5)[j, :n]
    return keep, kidx, n_keep, voted


def det_record(dets, n, top_cap):
    """[top_cap, 6] and a count -> [top_cap * 6 + 1]: rows at and beyond the clamped count +0.0, the clamped count as a float last"""
    n = clamp_count(n, top_cap)
    rec = np.zeros(top_cap * 6 + 1, F32)
    rec[:n * 6] = np.asarray(dets, F32)[:n].reshape(-1)
    rec[-1] = F32(n)
    return rec


# ---- C8I -----------------------------------------------------------------------------------------------------------------------------------
def c8i_pitch(rows):
    return round_up(rows, 128)


def c8i_pack(x, lane_fill=0.0, row_fill=0.0):
    """[B, C, H, W] -> [Cb][pitch][8]: element (b, c, y, x) at ((c / 8) * pitch + (b * H + y) * W + x) * 8 + c % 8"""
    x = np.asarray(x, F32)
    B, C, H, W = x.shape
    rows = B * H * W
    out = np.full((cdiv(C, 8), c8i_pitch(rows), 8), row_fill, F32)
    out[:, :rows, :] = lane_fill
    for c in range(C):
        out[c // 8, :rows, c % 8] = x[:, c].reshape(-1)
    return out


def c8i_unpack(m, B, C, H, W):
    m = np.asarray(m)
    return np.stack([m[c // 8, :B * H * W, c % 8].reshape(B, H, W) for c in range(C)], 1)


def pixel_major(x):
    """[C = 8 Cb, H, W] -> [H * W][Cb * 8]: channel c of pixel (y, x) at (y * W + x) * Cb * 8 + c"""
    x = np.asarray(x, F32)
    C, H, W = x.shape
    out = np.empty((H * W, C), F32)
    for c in range(C):
        out[:, c] = x[c].reshape(-1)
    return out


def mosaic_dims(cap, H, W, mx):
    return cdiv(cap, mx) * (H + 1), mx * (W + 1)


def mosaic_pack(x, cap, mx, fill=0.0):
    """[N, C = 8 Cb, H, W] -> the C8P image of a mosaic laid out for cap maps, mx per mosaic row: map b's pixel (y, x) at image pixel
    ((b / mx) * (H + 1) + y, (b % mx) * (W + 1) + x); everything else (separator rows and columns, cells of maps >= N, halo) `fill`"""
    x = np.asarray(x, F32)
    N, C, H, W = x.shape
    rows, cols = mosaic_dims(cap, H, W, mx)
    out = np.full((cdiv(C, 8), act_hp(rows), act_wp(cols), 8), fill, F32)
    for b in range(N):
        y0, x0 = (b // mx) * (H + 1) + 1, (b % mx) * (W + 1) + 1
        for c in range(C):
            out[c // 8, y0:y0 + H, x0:x0 + W, c % 8] = x[b, c]
    return out


def im2col3(img, KH, KW, stride, pad, row_fill=0.0):
    """[3, H, W] -> [round_up(KH * KW * 3, 64) / 8][pitch][8]: row = output pixel oy * OW + ox, k = (ky * KW + kx) * 3 + c; k beyond
    KH * KW * 3 and taps outside the image +0.0; rows beyond OH * OW `row_fill`"""
    img = np.asarray(img, F32)
    _, H, W = img.shape
    OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    out = np.full((round_up(KH * KW * 3, 64) // 8, c8i_pitch(OH * OW), 8), row_fill, F32)
    out[:, :OH * OW, :] = 0
    for oy in range(OH):
        for ox in range(OW):
            for ky in range(KH):
                for kx in range(KW):
                    iy, ix = oy * stride - pad + ky, ox * stride - pad + kx
                    if 0 <= iy < H and 0 <= ix < W:
                        for c in range(3):
                            k = (ky * KW + kx) * 3 + c
                            out[k // 8, oy * OW + ox, k % 8] = img[c, iy, ix]
    return out
