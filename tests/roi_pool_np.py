"""The layouts and references of the trunk-side ROI poolings and of the L2 normalisation behind them (multipathnet_amd/csrc/dense.h:
roi_pool_c8, roi_pool_c8_rmq, roi_pool_pm, roi_pool_pm_rmq, build_vmax_tables(_pm), l2norm_scale_c8, mul_const_c8), restated in NumPy for
tests/test_gpu_roi_pool_numerics.py (test infrastructure; checked on the CPU by tests/test_roi_pool_ref_cpu.py).  The bin geometry, the
float64 pooling, the ROI list and the value classes are tests/graph_pool_np.py's; this file adds the C8P / C8 / pixel-major layouts, the
arg-max and range-max-table references, the float64 normalisation, NumPy fp32 restatements of the two summation orders the kernels
document, and the input sets of the GPU file.

The derived bound of y = x * mul / sqrt(S + 1e-10), S = sum of K squares, evaluated in fp32 (u = 2^-24, every operation correctly rounded):
each square carries one rounding and the sum of K non-negative terms K - 1 more, in ANY order, so S32 = S (1 + t1) with
|t1| <= g(K) = K u / (1 - K u); the float constant 1e-10f and the addition add two more roundings to a positive sum: g = g(K + 2).  The
square root halves a relative error — |(1 + t)^(-1/2) - 1| <= g / 2 * (1 + g) for g < 1/2 — and rounds once; the in-place forms then divide and
multiply (two roundings: (v / d) * mul), the scale vector divides once (mul / d).  Hence
    |y32 - y64| <= (g / 2 * (1 + g) + (1 + ops) u) * |y64|,   ops = 2 in place, 1 for the scale,
plus one more u for rounding y64's own inputs' product to fp32 being exact here (x and mul are fp32 numbers): nothing to add.  A zero y64 has
a zero bound: 0 / d * mul is exactly 0.  K counts every lane that is summed, the +0 pad lanes included (they add nothing, so K is generous).
Sums that overflow fp32 are outside the bound (the float64 sum does not overflow); they are pinned to the restatement's bits instead."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_pool_np as G  # noqa: E402

F32, F64 = np.float32, np.float64
U24 = 2.0 ** -24
SENT = 0x7FA5A5A5  # a quiet NaN no arithmetic produces
SENT_F = np.array([SENT], np.uint32).view(F32)[0]
HALO = F32(2.0 ** 100)  # halo and pitch padding of a feature plane: finite, above every real value (`>` is blind to a NaN halo)
EPS32 = F32(1e-10)

roi_bins, roi_pool64, roi_table, value_class = G.roi_bins, G.roi_pool64, G.roi_table, G.value_class


def cdiv(a, b):
    return (a + b - 1) // b


def round_up(a, b):
    return cdiv(a, b) * b


def lin_mp(N):
    return round_up(N, 128)


def act_hp(H):
    return cdiv(H, 16) * 16 + 2


def act_wp(W):
    return cdiv(W, 32) * 32 + 2


def act_elems(C, H, W):
    return cdiv(C, 8) * act_hp(H) * act_wp(W) * 8


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def vmax_levels(H):
    """L: the levels k >= 1 with 2^k <= H"""
    L = 0
    while (2 << L) <= H:
        L += 1
    return L


# ---- layouts -----------------------------------------------------------------------------------------------------------------------------
def c8p_pack(x, halo=HALO):
    """[C, H, W] -> the C8P map [Cb][Hp][Wp][8]: pixel (y, x) of channel c at ((c / 8 * Hp + y + 1) * Wp + x + 1) * 8 + c % 8.  Halo and pitch
    padding hold `halo` in all 8 lanes; the pad lanes of a ragged last block hold +0 on the interior (the C8P contract)."""
    x = np.asarray(x, F32)
    C, H, W = x.shape
    out = np.full((cdiv(C, 8), act_hp(H), act_wp(W), 8), halo, F32)
    out[:, 1:H + 1, 1:W + 1, :] = 0
    for c in range(C):
        out[c // 8, 1:H + 1, 1:W + 1, c % 8] = x[c]
    return out


def c8p_unpack(m, C, H, W):
    """the interior of a C8P map -> [Cb * 8, H, W] (pad lanes included)"""
    m = np.asarray(m).reshape(cdiv(C, 8), act_hp(H), act_wp(W), 8)
    return np.ascontiguousarray(m[:, 1:H + 1, 1:W + 1, :].transpose(0, 3, 1, 2)).reshape(cdiv(C, 8) * 8, H, W)


def pm_unpack(m, C, H, W):
    """a pixel-major map [y][x][Cb * 8] (channel c of pixel (y, x) at (y * W + x) * Cb * 8 + c) -> [Cb * 8, H, W]"""
    return np.ascontiguousarray(np.asarray(m).reshape(H, W, cdiv(C, 8) * 8).transpose(2, 0, 1))


def c8_index(cb, b, n, lane, PP, Mp):
    """element (roi n, channel cb * 8 + lane, bin b) of the C8 matrix the poolings write"""
    return ((cb * PP + b) * Mp + n) * 8 + lane


def c8_unpack(xc8, C, PP, Mp):
    """the C8 matrix [Cb * PP][Mp][8] -> [Mp, Cb * 8, PP] (pad lanes and pad rows included)"""
    Cb = cdiv(C, 8)
    a = np.asarray(xc8).reshape(Cb, PP, Mp, 8)
    return np.ascontiguousarray(a.transpose(2, 0, 3, 1)).reshape(Mp, Cb * 8, PP)


def c8_pack(p, Mp, row_fill=SENT_F):
    """[N, Cb * 8, PP] -> [Cb * PP][Mp][8], rows n >= N `row_fill`"""
    p = np.asarray(p, F32)
    N, C8, PP = p.shape
    out = np.full((C8 // 8, PP, Mp, 8), row_fill, F32)
    out[:, :, :N, :] = p.reshape(N, C8 // 8, 8, PP).transpose(1, 3, 0, 2)
    return out.reshape(C8 // 8 * PP, Mp, 8)


# ---- references --------------------------------------------------------------------------------------------------------------------------
def roi_argmax(feat, rois, PH, PW, scale, rule):
    """int32 [N, C, PH, PW]: y * W + x of the FIRST maximum of each bin in row-major order (NaNs ignored); -1 for an empty bin and for a bin
    that holds nothing above -inf (only NaN and -inf: `v > m` from -inf never fires)"""
    feat = np.asarray(feat, F64)
    C, H, W = feat.shape
    fs = np.where(np.isnan(feat), -np.inf, feat)
    rois = np.asarray(rois, F32)
    out = np.full((rois.shape[0], C, PH, PW), -1, np.int32)
    for n, r in enumerate(rois):
        rows, cols = roi_bins(r, scale, H, W, PH, PW, rule)
        for i, (y0, y1) in enumerate(rows):
            for j, (x0, x1) in enumerate(cols):
                if y1 > y0 and x1 > x0:
                    w = fs[:, y0:y1, x0:x1].reshape(C, -1)
                    k = w.argmax(axis=1)  # the first occurrence
                    idx = (y0 + k // (x1 - x0)) * W + x0 + k % (x1 - x0)
                    out[n, :, i, j] = np.where(w.max(axis=1) > -np.inf, idx, -1)
    return out


def vmax_tables64(feat):
    """float64 [L + 1, C, H, W]: T_k[y][x] = max over rows y .. min(y + 2^k, H) - 1, NaNs ignored (a range of only NaN stays NaN); T_0 = the map"""
    feat = np.asarray(feat, F64)
    C, H, W = feat.shape
    L = vmax_levels(H)
    out = np.empty((L + 1, C, H, W))
    out[0] = feat
    for k in range(1, L + 1):
        for y in range(H):
            w = feat[:, y:min(y + (1 << k), H), :]
            allnan = np.isnan(w).all(axis=1)
            out[k, :, y, :] = np.where(allnan, np.nan, np.where(np.isnan(w), -np.inf, w).max(axis=1))
    return out


def l2norm64(x, mul):
    """x [N, K] -> (x * mul / sqrt(sum x^2 + 1e-10), mul / sqrt(sum x^2 + 1e-10)) in float64"""
    x = np.asarray(x, F64)
    d = np.sqrt((x * x).sum(axis=1) + 1e-10)
    return x * float(mul) / d[:, None], float(mul) / d


def l2norm_bound(ref, K, ops):
    """the bound of the header on |y32 - y64| for a sum of K squares; ops = 2 for (v / d) * mul, 1 for mul / d"""
    g = (K + 2) * U24 / (1.0 - (K + 2) * U24)
    return (0.5 * g * (1.0 + g) + (1 + ops) * U24) * np.abs(np.asarray(ref, F64))


def l2norm_c8_f32(xc8, N, mul, per=49):
    """l2norm_scale_c8's documented order on a C8 matrix [nrec][Mp][8]: per group of 49 records, sequentially over the records and over
    their 8 lanes with separately rounded squares; the group sums added in order; + 1e-10f; sqrtf; then (v / d) * mul.  Returns the matrix
    with rows < N scaled (the others untouched)."""
    x = np.array(xc8, F32)
    nrec = x.shape[0]
    v = x[:, :N, :]
    with np.errstate(all="ignore"):
        tot = np.zeros(N, F32)
        for g0 in range(0, nrec, per):
            ss = np.zeros(N, F32)
            for r in range(g0, min(nrec, g0 + per)):
                for e in range(8):
                    ss = ss + v[r, :, e] * v[r, :, e]
            tot = tot + ss
        d = np.sqrt(tot + EPS32)
        y = (v / d[None, :, None]) * F32(mul)
    assert y.dtype == F32 and d.dtype == F32
    x[:, :N, :] = y
    return x


def _butterfly(s):
    """ss += shfl_xor(ss, off) for off = 32 .. 1 over the last axis (64 lanes); every lane ends with the same tree's value"""
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[..., idx ^ off]
    return s


def l2norm_fused_f32(pooled, mul):
    """the fused form's documented order on pooled values [N, Cb * 8, PP] (pad lanes +0): per (roi, bin, 256-channel slice) each lane adds
    its four squares in lane order, then the xor butterfly 32 .. 1; the finish adds the G = PP * ceil(Cb / 32) partial sums ([bin][slice])
    lane-strided (g = lane, lane + 64, ..), then the butterfly, d = sqrtf(ss + 1e-10f).  Returns ((v / d) * mul, mul / d)."""
    p = np.asarray(pooled, F32)
    N, C8, PP = p.shape
    Cq = cdiv(C8, 256)
    m = np.zeros((N, Cq * 256, PP), F32)
    m[:, :C8, :] = p
    m = m.reshape(N, Cq, 64, 4, PP).transpose(0, 4, 1, 2, 3)  # [n][bin][slice][lane][e]
    with np.errstate(all="ignore"):
        ss = m[..., 0] * m[..., 0]
        for e in (1, 2, 3):
            ss = ss + m[..., e] * m[..., e]
        part = _butterfly(ss)[..., 0].reshape(N, PP * Cq)
        Gn = PP * Cq
        pad = np.zeros((N, round_up(Gn, 64)), F32)
        pad[:, :Gn] = part
        pad = pad.reshape(N, -1, 64)
        acc = np.zeros((N, 64), F32)
        for t in range(pad.shape[1]):
            acc = acc + pad[:, t, :]
        d = np.sqrt(_butterfly(acc)[:, 0] + EPS32)
        y = (p / d[:, None, None]) * F32(mul)
        s = F32(mul) / d
    assert y.dtype == F32 and s.dtype == F32
    return y, s


# ---- the input sets of the GPU file ----------------------------------------------------------------------------------------------------------
MAPS = [(3, 1, 1), (8, 2, 37), (20, 9, 3), (40, 21, 34), (16, 33, 40), (264, 9, 11)]
MAP_N = {(3, 1, 1): (1, 3, 5, 130), (8, 2, 37): (1, 3, 5, 130), (20, 9, 3): (3, 5), (40, 21, 34): (5,), (16, 33, 40): (3,), (264, 9, 11): (5, 130)}
SCALES = (1.0, 0.25, 0.0625)
BINS_MAP, OTHER_BINS = (40, 21, 34), ((6, 6), (1, 1), (3, 2))
FINITE_KINDS = ("mixed", "neg", "quant")


def odd_pitch(N):
    """a row pitch >= N that is a multiple of 4 (the quad staging writes whole ROI quads' lines) and of no 128"""
    return round_up(N, 8) + 8


def make_map(kind, C, H, W, seed):
    """mixed: mixed sign, magnitudes 2^-6 .. 2^6.  neg: all negative (an empty bin's 0 is then above every maximum).  quant: multiples of
    0.25 in [-2, 2] (ties: the first-maximum rule).  zero: all +0.  huge: mixed * 2^70 (every square overflows).  edge: mixed with +-0 and
    +-inf sprinkled in and NaN at a fifth of the cells (so at the head of bins' row ranges and of their power-of-two sub-ranges), all of
    row 0 of channel 0, all of column min(1, W - 1) of channel 1 and the whole of channel 2 (every window)."""
    rng = np.random.default_rng([C, H, W, seed, len(kind)])
    x = G.mixed_sign(rng, (C, H, W))
    if kind == "neg":
        x = -np.abs(x)
    elif kind == "quant":
        x = (rng.integers(-8, 9, (C, H, W)) * 0.25).astype(F32)
    elif kind == "zero":
        x = np.zeros((C, H, W), F32)
    elif kind == "huge":
        x = x * F32(2.0 ** 70)
    elif kind == "edge":
        r = rng.random((C, H, W))
        x[r < 0.20] = np.nan
        x[(r >= 0.20) & (r < 0.24)] = 0.0
        x[(r >= 0.24) & (r < 0.28)] = -0.0
        x[(r >= 0.28) & (r < 0.31)] = np.inf
        x[(r >= 0.31) & (r < 0.36)] = -np.inf
        x[0, 0, :] = np.nan
        if C > 1:
            x[1, :, min(1, W - 1)] = np.nan
        if C > 2:
            x[2] = np.nan
    else:
        assert kind == "mixed"
    return x.astype(F32)


def make_rois(N, H, W, scale, off, rule, zero_row=False):
    """N rows (col0, x1, y1, x2, y2): graph_pool_np.roi_table's list starting at entry `off`, with (N >= 3) a window of +-1e6, (N >= 5) a
    window at +1e6 wholly outside and the x4 region of a box filling the image (window = the whole map).  zero_row: row 0 wholly outside
    (an all-empty ROI under rule 0).  Column 0 is left 1."""
    rng = np.random.default_rng([N, H, W, off, rule])
    t = roi_table(rng, 11 + N, H, W, scale)[off % 11:off % 11 + N].copy()
    iw, ih = W / scale, H / scale
    if N >= 3:
        t[1, 1:] = (-1e6, -1e6, 1e6, 1e6)
    if N >= 5:
        t[3, 1:] = (1e6, 1e6, 1e6 + 50, 1e6 + 50)
        t[4, 1:] = (1 - 1.5 * iw, 1 - 1.5 * ih, 2.5 * iw, 2.5 * ih)
    if zero_row:
        t[0, 1:] = (3 * iw + 100, 3 * ih + 100, 4 * iw + 100, 4 * ih + 100)
    return t.astype(F32)


def foveal_table(rois, region, col0=np.nan):
    """the [N, 4, 5] table a roi_stride of 20 walks: `rois` at region `region`, other boxes (shifted and grown) at the three others"""
    N = rois.shape[0]
    t = np.empty((N, 4, 5), F32)
    for r in range(4):
        t[:, r, :] = rois
        if r != region:
            t[:, r, 1:] += F32(3.0 + r) * np.array([1, 2, 5, 3], F32)
    t[:, :, 0] = col0
    return t


def pool_cases():
    """(C, H, W, N, kind, rule, scale, Mp, roi_stride, region, PH, PW): every map x its N list x both rules, on the edge map and on one of
    the finite kinds in rotation; scale, pitch, ROI stride and Foveal region rotate with the case; 7 x 7 bins, and on one map 6 x 6, 1 x 1, 3 x 2"""
    out = []
    for si, (C, H, W) in enumerate(MAPS):
        for ni, N in enumerate(MAP_N[(C, H, W)]):
            for rule in (0, 1):
                k = si + ni + rule
                for kind in ("edge", FINITE_KINDS[k % 3]):
                    if N == 130 and C > 8 and kind != "edge":
                        continue  # (the widest matrix once per rule)
                    out.append((C, H, W, N, kind, rule, SCALES[k % 3], odd_pitch(N) if (ni + rule) % 2 else 0, 20 if k % 2 else 5, (k // 2) % 4, 7, 7))
    C, H, W = BINS_MAP
    for bi, (PH, PW) in enumerate(OTHER_BINS):
        for rule in (0, 1):
            out.append((C, H, W, 5, "edge" if rule else "quant", rule, SCALES[(bi + rule) % 3], 0, 5, 0, PH, PW))
    return out


def norm_cases():
    """(C, H, W, N, kind, rule, scale, Mp, mul) of the normalising forms: finite maps, the all-zero map and the overflowing one"""
    out = []
    for si, (C, H, W, Ns) in enumerate([(3, 1, 1, (1, 130)), (8, 2, 37, (3, 130)), (20, 9, 3, (5,)), (40, 21, 34, (5,)), (16, 33, 40, (3,)),
                                        (264, 9, 11, (5, 130))]):
        for ni, N in enumerate(Ns):
            rule = (si + ni) % 2
            out.append((C, H, W, N, FINITE_KINDS[(si + ni) % 3], rule, SCALES[(si + ni) % 3], odd_pitch(N) if ni % 2 == 0 else 0, 1000.0 if si % 2 else 0.37))
    out.append((20, 9, 3, 3, "zero", 1, 0.25, 0, 1000.0))
    out.append((264, 9, 11, 5, "huge", 0, 1.0, 0, 1000.0))
    return out


@functools.lru_cache(maxsize=None)
def pool_inputs(C, H, W, N, kind, rule, scale, PH=7, PW=7, zero_row=False):
    """(map [C, H, W] fp32, rois [N, 5] fp32, pooled float64 [N, C, PH, PW]) — computed once per case, shared, never written"""
    feat = make_map(kind, C, H, W, 7)
    rois = make_rois(N, H, W, scale, C + H + N, rule, zero_row)
    ref = roi_pool64(feat, rois, PH, PW, scale, rule)
    for a in (feat, rois, ref):
        a.setflags(write=False)
    return feat, rois, ref


def pooled_padded(ref, C):
    """float64 [N, C, PH, PW] -> fp32 [N, Cb * 8, PP] with +0 pad lanes: what the poolings leave in rows < N of the C8 matrix"""
    N = ref.shape[0]
    p = np.zeros((N, cdiv(C, 8) * 8, ref.shape[2] * ref.shape[3]), F32)
    p[:, :C, :] = ref.reshape(N, C, -1).astype(F32)
    return p


L2_CASES = [(1, 1, 8), (50, 5, 16), (98, 130, 0), (120, 3, 24), (147, 130, 144)]  # (n_records, N, Mp): n_records on and off a multiple of 49


def l2_inputs(nrec, N, Mp):
    """a C8 matrix [nrec][Mp][8]: mixed-sign values with exact zeros in rows < N, the sentinel in the others"""
    Mp = Mp or lin_mp(N)
    rng = np.random.default_rng([nrec, N, Mp, 3])
    x = np.full((nrec, Mp, 8), SENT_F, F32)
    v = G.mixed_sign(rng, (nrec, N, 8))
    v[rng.random((nrec, N, 8)) < 0.1] = 0
    x[:, :N, :] = v
    return x
