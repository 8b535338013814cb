"""The layouts and references of the head-training kernels (multipathnet_amd/csrc/train.h), restated in NumPy for
tests/test_gpu_train_kernels_numerics.py (test infrastructure).  Written from the header comments of train.h and dense.h, not from the
kernels: the C8 matrix, the packed linear weight with its `inner` permutation, the packed conv weight `wpk`, the C8P map; float64
references of the loss and its gradient, of dW, db and dx; the fp32 restatements of what the headers document operation by operation
(optim.sgd's chain, sgd_bias_kernel's summation order, dropout's scaling, the loss's reduction order); and the input sets of the GPU file,
so that tests/test_train_kernels_ref_cpu.py can show on the CPU that a plain fp32 evaluation of every one of them meets the bounds.

The derived bound of a length-n fp32 dot product r = sum a_i b_i: |r - r64| <= (n + 1) * 2^-23 * sum |a_i| |b_i|, for any summation order,
fused or unfused products and any faithfully rounded addition (hence 2^-23, not 2^-24): n - 1 additions and one product rounding per term,
each at most one unit of the running magnitude, which sum |a_i| |b_i| (1 + n u) bounds; n + 1 absorbs the second-order term for n u << 1."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dropout_np as D  # noqa: E402
import train_np as T  # noqa: E402

F32, F64 = np.float32, np.float64
U23 = 2.0 ** -23
SENT = 0x7FA5A5A5  # a quiet NaN no arithmetic produces: "not written" is told from "rewritten with the same value"
SENT_F = np.array([SENT], np.uint32).view(F32)[0]
MEAN4, STD4 = (0.01, -0.02, 0.03, 0.005), (0.1, 0.1, 0.2, 0.2)
SEED = 0x1234ABCD9E3779B1  # both 32-bit halves non-zero


def cdiv(a, b):
    return (a + b - 1) // b


def round_up(a, b):
    return cdiv(a, b) * b


def lin_np(N):
    return round_up(N, 128)


def k64(K):
    return round_up(K, 64)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def draw(rng, shape, zero_frac=0.1, positive=False):
    """fp32 values with magnitudes log-uniform in [2^-6, 2^3], random signs, and exact zeros: no subnormal, no overflow in any sum here"""
    v = np.exp2(rng.uniform(-6.0, 3.0, shape)).astype(F32)
    if not positive:
        v *= rng.choice(np.array([-1, 1], F32), shape)
    v[rng.random(shape) < zero_frac] = 0
    return v


# ---- layouts -----------------------------------------------------------------------------------------------------------------------------
def c8_pack(a, Mp, chunks=None, lane_fill=0.0, row_fill=0.0):
    """[M, N] -> the C8 matrix [chunks][Mp][8]: element (m, n) at ((n / 8) * Mp + m) * 8 + n % 8.  lane_fill: lanes n >= N of rows < M;
    row_fill: rows >= M."""
    a = np.asarray(a, F32)
    M, N = a.shape
    chunks = cdiv(N, 8) if chunks is None else chunks
    out = np.full((chunks, Mp, 8), row_fill, F32)
    out[:, :M, :] = lane_fill
    for n in range(N):
        out[n // 8, :M, n % 8] = a[:, n]
    return out


def c8_unpack(c8, M, N):
    c8 = np.asarray(c8)
    out = np.empty((M, N), c8.dtype)
    for n in range(N):
        out[:, n] = c8[n // 8, :M, n % 8]
    return out


def lin_k_index(K, inner):
    """[K64 / 8, 8] int64: the k that lane j of chunk q of a packed linear weight (and of its operand matrix) holds,
    k = ((q / inner) * 8 + j) * inner + q % inner; k >= K: a pad lane"""
    q = np.arange(k64(K) // 8)[:, None]
    j = np.arange(8)[None, :]
    return ((q // inner) * 8 + j) * inner + q % inner


def lin_valid(K, N, inner):
    """[K64 / 8, NP, 8] bool: the lanes of the pack that belong to the layer"""
    kidx = lin_k_index(K, inner)
    v = np.zeros((kidx.shape[0], lin_np(N), 8), bool)
    v[:, :N, :] = (kidx < K)[:, None, :]
    return v


def lin_pack(w, inner=1, fill=0.0):
    """[N, K] (Torch layout) -> [K64 / 8][NP][8], pad lanes `fill`"""
    w = np.asarray(w, F32)
    N, K = w.shape
    kidx = lin_k_index(K, inner)
    out = np.full((kidx.shape[0], lin_np(N), 8), fill, F32)
    ok = kidx < K
    for q in range(kidx.shape[0]):
        for j in range(8):
            if ok[q, j]:
                out[q, :N, j] = w[:, kidx[q, j]]
    return out


def lin_unpack(wpk, K, N, inner=1):
    wpk = np.asarray(wpk)
    kidx = lin_k_index(K, inner)
    out = np.empty((N, K), wpk.dtype)
    for q in range(kidx.shape[0]):
        for j in range(8):
            if kidx[q, j] < K:
                out[:, kidx[q, j]] = wpk[q, :N, j]
    return out


def bias_pack(b, fill=0.0):
    b = np.asarray(b, F32)
    out = np.full(lin_np(b.shape[0]), fill, F32)
    out[:b.shape[0]] = b
    return out


def x_pack(x, inner, Mp, lane_fill=0.0, row_fill=0.0):
    """[M, K] -> the operand matrix of a packed linear weight, [K64 / 8][Mp][8]: lane j of chunk q holds column lin_k_index[q, j]"""
    x = np.asarray(x, F32)
    M, K = x.shape
    kidx = lin_k_index(K, inner)
    out = np.full((kidx.shape[0], Mp, 8), row_fill, F32)
    out[:, :M, :] = lane_fill
    for q in range(kidx.shape[0]):
        for j in range(8):
            if kidx[q, j] < K:
                out[q, :M, j] = x[:, kidx[q, j]]
    return out


def conv_coutp(Cout):
    return round_up(Cout, 128)


def conv_valid(Cin, Cout):
    """[Cin8 / 8, 9, CoutP, 8] bool"""
    v = np.zeros((cdiv(Cin, 8), 9, conv_coutp(Cout), 8), bool)
    ci = np.arange(cdiv(Cin, 8))[:, None] * 8 + np.arange(8)[None, :]
    v[:, :, :Cout, :] = (ci < Cin)[:, None, None, :]
    return v


def conv_pack(w, fill=0.0):
    """[Cout, Cin, 3, 3] -> `wpk` [Cin8 / 8][9][CoutP][8]: tap = ky * 3 + kx, lane j of chunk c = input channel 8 c + j"""
    w = np.asarray(w, F32)
    Cout, Cin = w.shape[:2]
    out = np.full((cdiv(Cin, 8), 9, conv_coutp(Cout), 8), fill, F32)
    w9 = w.reshape(Cout, Cin, 9)
    for ci in range(Cin):
        out[ci // 8, :, :Cout, ci % 8] = w9[:, ci, :].T
    return out


def conv_unpack(wpk, Cin, Cout):
    wpk = np.asarray(wpk)
    out = np.empty((Cout, Cin, 9), wpk.dtype)
    for ci in range(Cin):
        out[:, ci, :] = wpk[ci // 8, :, :Cout, ci % 8].T
    return out.reshape(Cout, Cin, 3, 3)


def act_hp(H):
    return cdiv(H, 16) * 16 + 2


def act_wp(W):
    return cdiv(W, 32) * 32 + 2


def c8p_pack(x, fill=0.0):
    """[C, H, W] -> the C8P map [Cb][Hp][Wp][8]: pixel (y, x) of channel c at ((c / 8 * Hp + y + 1) * Wp + x + 1) * 8 + c % 8; halo, pitch
    padding and pad channels `fill`"""
    x = np.asarray(x, F32)
    C, H, W = x.shape
    out = np.full((cdiv(C, 8), act_hp(H), act_wp(W), 8), fill, F32)
    for c in range(C):
        out[c // 8, 1:H + 1, 1:W + 1, c % 8] = x[c]
    return out


def c8p_interior(C, H, W):
    """bool mask of the records relu_mask_c8p touches: the H x W interior of every plane, all 8 lanes"""
    m = np.zeros((cdiv(C, 8), act_hp(H), act_wp(W), 8), bool)
    m[:, 1:H + 1, 1:W + 1, :] = True
    return m


# ---- optim.sgd, each operation rounded on its own ------------------------------------------------------------------------------------------
def sgd_f32(w, v, dw, lr, mom, wd):
    """gr = f32(dW + f32(wd * w)); v' = f32(f32(mom * v) + gr); w' = f32(w - f32(lr * v')) -> (w', v')"""
    w, v, dw = np.asarray(w, F32), np.asarray(v, F32), np.asarray(dw, F32)
    lr, mom, wd = F32(lr), F32(mom), F32(wd)
    with np.errstate(all="ignore"):
        gr = dw + wd * w
        v2 = mom * v + gr
        w2 = w - lr * v2
    assert gr.dtype == F32 and v2.dtype == F32 and w2.dtype == F32
    return w2, v2


def sgd_bias_f32(b, vb, db, lr, mom):
    """v' = f32(f32(mom * v) + db); b' = f32(b - f32(lr * v')): biases never decay"""
    b, vb, db = np.asarray(b, F32), np.asarray(vb, F32), np.asarray(db, F32)
    v2 = F32(mom) * vb + db
    return b - F32(lr) * v2, v2


def bias_sum_f32(g):
    """sgd_bias_kernel's documented order on g [B, N]: 32 slot sums from +0 over m = slot, slot + 32, ... ascending, then the tree
    16, 8, 4, 2, 1 (part[s] += part[s + w])"""
    g = np.asarray(g, F32)
    B, N = g.shape
    part = np.zeros((32, N), F32)
    for m in range(B):
        part[m % 32] = part[m % 32] + g[m]
    w = 16
    while w:
        part[:w] = part[:w] + part[w:2 * w]
        w //= 2
    return part[0].copy()


def seq_dot_f32(a, b):
    """a [n, P], b [n, Q] -> [P, Q]: sum_i a[i, p] b[i, q] by a plain fp32 chain, i ascending, product and sum rounded separately"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    acc = np.zeros((a.shape[1], b.shape[1]), F32)
    for i in range(a.shape[0]):
        acc = acc + a[i][:, None] * b[i][None, :]
    return acc


def dot_bound(a, b, n, extra=1):
    """(n + extra) * 2^-23 * sum_i |a_i| |b_i| for a [n, P], b [n, Q] -> [P, Q], float64"""
    return (n + extra) * U23 * (np.abs(np.asarray(a, F64)).T @ np.abs(np.asarray(b, F64)))


# ---- the loss ------------------------------------------------------------------------------------------------------------------------------
def clamp_labels(labels, C):
    return np.clip(np.asarray(labels, np.int64), 0, C - 1)


def loss_ref64(head, C, K, k, rois, gt, labels, mean, std, norm, bbox_weight):
    """train.h train_loss in float64 on the fp32 inputs -> (loss [2], g [B, (K + 4) C])"""
    head = np.asarray(head, F64)
    B = head.shape[0]
    y = clamp_labels(labels, C)
    z = head[:, k * C:(k + 1) * C]
    mx = z.max(1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(z - mx).sum(1))
    L_cls = (lse - z[np.arange(B), y]).sum() / B
    g = np.zeros_like(head)
    soft = np.exp(z - lse[:, None])
    soft[np.arange(B), y] -= 1.0
    g[:, k * C:(k + 1) * C] = soft / B
    bw = float(F32(bbox_weight))
    t, fg = T.targets(np.asarray(rois, F64), np.asarray(gt, F64), y, np.asarray(mean, F32).astype(F64), np.asarray(std, F32).astype(F64) if norm else None)
    idx = np.nonzero(fg)[0]
    L_box = 0.0
    if idx.size:
        cols = K * C + 4 * y[idx][:, None] + np.arange(4)[None, :]
        d = head[idx[:, None], cols] - t[idx]
        L_box = bw * np.where(np.abs(d) < 1.0, 0.5 * d * d, np.abs(d) - 0.5).sum() / B
        g[idx[:, None], cols] = bw / B * np.clip(d, -1.0, 1.0)
    return np.array([L_cls, L_box]), g


def block_reduce_f32(rows):
    """train_loss_kernel's documented reduction of per-row terms [B]: thread t adds rows t, t + 256, ... ascending from +0, then the tree
    128, 64, ..., 1"""
    rows = np.asarray(rows, F32)
    s = np.zeros(256, F32)
    for i in range(rows.shape[0]):
        s[i % 256] = s[i % 256] + rows[i]
    w = 128
    while w:
        s[:w] = s[:w] + s[w:2 * w]
        w //= 2
    return s[0]


def loss_f32(head, C, K, k, rois, gt, labels, mean, std, norm, bbox_weight):
    """The same chain in NumPy fp32, every operation rounded on its own, sums in the documented order (the row's exp sum: c ascending):
    the yardstick beside float64 for the parts that go through exp and log -> (loss [2] fp32, g [B, (K + 4) C] fp32)"""
    head = np.asarray(head, F32)
    B = head.shape[0]
    y = clamp_labels(labels, C)
    r, t = np.asarray(rois, F32), np.asarray(gt, F32)
    invB, gbox = F32(1.0) / F32(B), F32(bbox_weight) / F32(B)
    mean, std = np.asarray(mean, F32), np.asarray(std, F32)
    g = np.zeros_like(head)
    box_rows = np.zeros(B, F32)
    half, rows = F32(0.5), np.arange(B)
    with np.errstate(all="ignore"):  # every step elementwise over the rows: the same roundings as a row-by-row loop
        z = head[:, k * C:(k + 1) * C]
        mx = z.max(1)
        e = np.exp(z - mx[:, None])
        s = np.zeros(B, F32)
        for c in range(C):
            s = s + e[:, c]
        cls_rows = (mx + np.log(s)) - z[rows, y]
        one = np.zeros((B, C), F32)
        one[rows, y] = 1
        g[:, k * C:(k + 1) * C] = (e * (F32(1.0) / s)[:, None] - one) * invB
        xc, yc, w, h = (r[:, 0] + r[:, 2]) * half, (r[:, 1] + r[:, 3]) * half, r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
        xtc, ytc, wt, ht = (t[:, 0] + t[:, 2]) * half, (t[:, 1] + t[:, 3]) * half, t[:, 2] - t[:, 0], t[:, 3] - t[:, 1]
        tg = np.stack([(xtc - xc) / w, (ytc - yc) / h, np.log(wt / w), np.log(ht / h)], 1).astype(F32)
        if norm:
            tg = (tg - mean[None, :]) / std[None, :]
        fg = np.nonzero(y > 0)[0]
        cols = K * C + 4 * y[fg][:, None] + np.arange(4)[None, :]
        d = head[fg[:, None], cols] - tg[fg]
        a = np.abs(d)
        term = np.where(a < 1, half * d * d, a - half).astype(F32)
        row = np.zeros(fg.shape[0], F32)
        for j in range(4):
            row = row + term[:, j]
        box_rows[fg] = row
        g[fg[:, None], cols] = gbox * np.where(d < -1, F32(-1), np.where(d > 1, F32(1), d)).astype(F32)
    assert g.dtype == F32 and cls_rows.dtype == F32 and tg.dtype == F32
    return np.array([block_reduce_f32(cls_rows) * invB, block_reduce_f32(box_rows) * gbox], F32), g


# ---- dropout -------------------------------------------------------------------------------------------------------------------------------
def dropout_f32(x, rate, seed, step, layer):
    """train.h dropout_c8 on x [B, N]: kept (word >= floor(rate * 2^32)) f32(x * scale), dropped +0.0 -> (y, keep)"""
    x = np.asarray(x, F32)
    keep = D.keep_mask(seed, step, layer, x.shape[0], x.shape[1], rate)
    with np.errstate(all="ignore"):
        y = np.where(keep, x * D.scale(rate), F32(0)).astype(F32)
    return y, keep


# ---- the GPU file's input sets -------------------------------------------------------------------------------------------------------------
WGRAD_N = (1, 35, 128, 129)
WGRAD_KI = ((8, 1), (96, 1), (264, 1), (48, 3), (1568, 49))
WGRAD_B = (1, 2, 3, 33, 130)
WGRAD_RAGGED = (35, (264, 1), 33)


def wgrad_cases():
    """one pass over each axis with the others at their ragged value, and the full N x B product at the cheap (K, inner) = (48, 3)"""
    n_, ki_, b_ = WGRAD_RAGGED
    cases = [(N, ki_, b_) for N in WGRAD_N] + [(n_, ki, b_) for ki in WGRAD_KI] + [(n_, ki_, B) for B in WGRAD_B]
    cases += [(N, (48, 3), B) for N in WGRAD_N for B in WGRAD_B]
    cases += [(129, (1568, 49), 130), (1, (8, 1), 1)]
    out = []
    for c in cases:
        if c not in out:
            out.append(c)
    return [(N, K, inner, B) for N, (K, inner), B in out]


def wgrad_inputs(N, K, inner, B):
    rng = np.random.default_rng([N, K, inner, B, 1])
    return draw(rng, (B, N)), draw(rng, (B, K))  # g, x


BIAS_N = (1, 7, 8, 9, 35, 130)
BIAS_B = (1, 31, 32, 33, 100)


def bias_inputs(N, B):
    return draw(np.random.default_rng([N, B, 2]), (B, N))


DGRAD_N = (1, 2, 3, 7, 35, 130)
DGRAD_K = (8, 96, 264)
DGRAD_B = (1, 31, 32, 33, 70)


def dgrad_cases():
    return [(N, K, B) for N in DGRAD_N for K in DGRAD_K for B in DGRAD_B]


def dgrad_inputs(N, K, B):
    """g [B, N], w [N, K], act [B, K] holding positive values, +0.0, -0.0, negative values, 2^-126 and NaN"""
    rng = np.random.default_rng([N, K, B, 3])
    g, w = draw(rng, (B, N)), draw(rng, (N, K))
    act = draw(rng, (B, K), zero_frac=0.0)
    pick = rng.integers(0, 10, (B, K))
    act[pick == 0] = 0.0
    act[pick == 1] = -0.0
    act[pick == 2] = F32(2.0 ** -126)
    act[pick == 3] = np.nan
    return g, w, act


LOSS_CKK = ((2, 1, 0), (7, 1, 0), (21, 1, 0), (81, 1, 0), (7, 3, 0), (7, 3, 1), (7, 3, 2), (81, 2, 1))
LOSS_B = (1, 2, 255, 256, 257, 300)


def loss_inputs(C, K, k, B, all_bg=False, saturated=False):
    """head [B, (K + 4) C], rois, gt [B, 4], labels [B]: foreground and background mixed, plus -3, C and C + 5"""
    rng = np.random.default_rng([C, K, k, B, 4])
    head = draw(rng, (B, (K + 4) * C))
    if saturated:
        head[:, :K * C] = rng.choice(np.array([-80, 80], F32), (B, K * C))
    xy = rng.uniform(1, 500, (B, 2))
    wh = rng.uniform(8, 200, (B, 2))
    rois = np.concatenate([xy, xy + wh], 1).astype(F32)
    gxy = xy + rng.uniform(-0.2, 0.2, (B, 2)) * wh
    gwh = wh * np.exp(rng.uniform(-0.3, 0.3, (B, 2)))
    gt = np.concatenate([gxy, gxy + gwh], 1).astype(F32)
    labels = np.where(rng.random(B) < 0.5, 0, rng.integers(1, C, B)).astype(np.int32)
    odd = np.array([-3, C, C + 5], np.int32)
    for i in range(min(B, 3)):  # the three out-of-range values where the batch has room for them
        labels[(i * 97 + B // 2) % B] = odd[i]
    if all_bg:
        labels[:] = 0
        labels[B // 2] = -3  # clamps to background
    return head, rois, gt, labels


BOUNDARY_D = np.array([1, -1, 1 - 2.0 ** -24, -(1 - 2.0 ** -24), 1 + 2.0 ** -23, -(1 + 2.0 ** -23), 0.0, -0.0], F32)


def loss_boundary_inputs(C, K, k, B):
    """norm = 0 and gt == roi: the targets are exactly 0, so d is the box output itself; every foreground row's four outputs walk
    BOUNDARY_D.  -> head, rois, gt, labels"""
    head, rois, _, labels = loss_inputs(C, K, k, B)
    y = clamp_labels(labels, C)
    n = 0
    for i in range(B):
        if y[i] > 0:
            for j in range(4):
                head[i, K * C + 4 * y[i] + j] = BOUNDARY_D[(n + j) % 8]
            n += 3
    return head, rois, rois.copy(), labels
