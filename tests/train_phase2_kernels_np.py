"""Layouts, restatements and input sets for tests/test_gpu_train_phase2_kernels_numerics.py (test infrastructure):
the kernels between MultiPathNet's mix layers and its conv block, one launch at a time — normalize_backward_kernel,
roi_pool_backward_add_kernel, int_to_float_kernel and linear_dgrad_c8 in the tower backward's prefix-launch form.  The Normalize
backward's order and bound are tests/train_phase2_np.py's (generalised to C % 8 != 0), the ROI windows tests/train_conv_kernels_np.py's.
tests/test_train_phase2_kernels_ref_cpu.py checks every claim made here on the CPU."""
import numpy as np

import train_conv_kernels_np as K
import train_kernels_np as R
import train_phase2_np as P2

F32, F64 = np.float32, np.float64
U23 = R.U23
SENT_F = R.SENT_F
cdiv = R.cdiv


# ---- one tower's conv5 slab: [ceil(C/8) * PP][Mp][8], record (c / 8) * PP + bin, row n, lane c % 8 --------------------------------
def slab_pack(a, Mp, fill=0.0):
    """[B, C, PP] -> the slab; pad lanes (c >= C) and rows >= B hold `fill`"""
    return K.roi_g_c8(a, Mp, fill=fill)


def slab_unpack(s, B, C, PP):
    s = np.asarray(s)
    out = np.empty((B, C, PP), s.dtype)
    for c in range(C):
        out[:, c, :] = s[(c // 8) * PP:(c // 8 + 1) * PP, :B, c % 8].T
    return out


def slab_real(B, C, PP, Mp):
    """bool, the slab's shape: the lanes the kernel may read and must write"""
    return slab_pack(np.ones((B, C, PP), F32), Mp, fill=0.0) > 0


# ---- nn.Normalize(2) x mul backward -------------------------------------------------------------------------------------------------
# (C, PP, B, Mp): the smallest shape; E = 8 with three real entries; E = 256 exactly; E = 320 with seven pad lanes in the last block;
# two ragged ones; the two networks' shapes; the product's chain length L = 98 at two rows
NORM_CASES = ((1, 1, 1, 1), (3, 1, 2, 5), (8, 32, 3, 3), (33, 8, 2, 4), (9, 7, 4, 4), (12, 49, 5, 8), (40, 49, 70, 128), (48, 49, 128, 128),
              (512, 49, 2, 2))
NORM_MUL = {(9, 7, 4, 4): 4.0, (12, 49, 5, 8): 0.37}   # every other case: 1000


def norm_mul(case):
    return NORM_MUL.get(tuple(case), P2.MUL)


def draw12(rng, shape, zero_frac=0.1, bits=12, emin=-6, emax=2):
    """fp32 values m * 2^(e - 11) with m in [2^11, 2^12) and e in [-6, 2]: at most 12 significant bits, magnitudes in [2^-6, 2^3), random
    signs, exact zeros.  A product of two has at most 24 bits and is a multiple of 2^-34; a partial sum of up to 2^7 of them stays below
    2^13, so product + partial spans fewer than 53 bits: float64 holds it exactly and rounding it to fp32 is the fused multiply-add."""
    m = rng.integers(2 ** (bits - 1), 2 ** bits, shape).astype(F64)
    v = (m * np.exp2(rng.integers(emin, emax + 1, shape) - (bits - 1.0))).astype(F32)
    v *= rng.choice(np.array([-1, 1], F32), shape)
    v[rng.random(shape) < zero_frac] = 0
    return v


def draw16(rng, shape, zero_frac=0.1):
    """The second bit-exact set.  A product of two draw12 values has at most 24 bits: it is an fp32 value, so fl(fl(x y) + acc) IS
    fma(x, y, acc) and the 12-bit set cannot tell a kernel without the fma from one with it.  Here: 16 significant bits, magnitudes in
    [2^-2, 2^2) — still multiples of 2^-17, products of up to 32 bits (rounded by a plain multiply) that are multiples of 2^-34 and below
    2^4, partial sums below 2^11: product + partial spans fewer than 53 bits, so the float64 emulation is still the fma exactly."""
    return draw12(rng, shape, zero_frac, bits=16, emin=-2, emax=1)


BIT_TIERS = ("bits", "bits16")


def norm_inputs(case, tier):
    """-> x, y, g [B, C, PP] fp32.  tier "bits" / "bits16": draw12 / draw16 operands; the last row (B >= 2) has x = y = 0 (s = mul / sqrt(1e-10f)), row 0
    (B >= 3) has g = 0.  "exact": integers in [-2, 2].  "derived": full-mantissa magnitudes in [2^-6, 2^3] (R.draw)."""
    C, PP, B, Mp = case
    rng = np.random.default_rng([C, PP, B, Mp, {"bits": 1, "exact": 2, "derived": 3, "bits16": 4}[tier]])
    shape = (B, C, PP)
    if tier in BIT_TIERS:
        x, y, g = ((draw12 if tier == "bits" else draw16)(rng, shape) for _ in range(3))
        if B >= 2:
            x[B - 1], y[B - 1] = 0, 0
        if B >= 3:
            g[0] = 0
    elif tier == "exact":
        x, y, g = (rng.integers(-2, 3, shape).astype(F32) for _ in range(3))
    else:
        x, y, g = (R.draw(rng, shape) for _ in range(3))
    return x, y, g


def normalize_backward_exact(x, y, g, mul):
    """the kernel's tail fed the float64 sums rounded once: for integer operands whose sums stay below 2^24 every partial sum of ANY order
    is exact, so this is what the device must give whatever its order — a dropped or doubled entry shows with no tolerance"""
    x64, y64, g64 = (np.asarray(a, F64) for a in (x, y, g))
    ss, d = (x64 * x64).sum((1, 2)), (y64 * g64).sum((1, 2))
    assert (ss < 2.0 ** 24).all() and (np.abs(y64 * g64).sum((1, 2)) < 2.0 ** 24).all()
    return P2.normalize_backward_tail(ss.astype(F32), d.astype(F32), y, g, mul)


# ---- the gather that continues the chain --------------------------------------------------------------------------------------------
def gather_chain(map0, g, argmax, n0, n1, W, rois5=None, PH=0, PW=0, scale=K.ROI_SCALE, rule=0, windows=False, dtype=F32):
    """ONE call of roi_pool_backward_add restated: map0 [C, H, W] -> the map after the call.  Per cell one chain in `dtype` (fp32: the
    kernel's) that starts at the cell's value: rows [n0, n1) ascending, bins ascending, one add per term with argmax == cell; argmax -1
    is skipped.  A cell no term reaches is not touched (its bits stay, -0.0 and a NaN's payload included).  windows: a bin counts only
    if the cell lies in its window (K.roi_windows, the forward's roi_bin_bounds)."""
    g, am = np.asarray(g, dtype), np.asarray(argmax).astype(np.int64)
    C, H, _ = map0.shape
    PP = am.shape[2]
    out = np.array(map0, dtype).reshape(C, H * W).copy()
    cs = np.arange(C)
    if windows:
        sel = np.nan_to_num(np.asarray(rois5, F32))   # (rows outside [n0, n1) may hold NaN: their windows are never used)
        hs, he, ws, we = K.roi_windows(sel, H, W, PH, PW, scale, rule)
    for n in range(n0, n1):
        for k in range(PP):
            i = am[n, :, k]
            ok = i >= 0
            if windows:
                ph, pw = divmod(k, PW)
                yy, xx = i // W, i % W
                ok = ok & (yy >= hs[n, ph]) & (yy < he[n, ph]) & (xx >= ws[n, pw]) & (xx < we[n, pw])
            out[cs[ok], i[ok]] = out[cs[ok], i[ok]] + g[n, ok, k]   # one term per channel: no index repeats
    return out.reshape(C, H, W)


def gather_bound(map0, g, argmax, n0, n1, W):
    """|fp32 chain - float64 chain| <= (terms + 1) * 2^-23 * (|start| + sum |g|) per cell: section 13.14's bound of the ordered sum with
    the start value as one more term"""
    cnt = gather_chain(np.zeros(np.shape(map0)), np.ones(np.shape(g)), argmax, n0, n1, W, dtype=F64)
    mag = gather_chain(np.abs(np.asarray(map0, F64)), np.abs(np.asarray(g, F64)), argmax, n0, n1, W, dtype=F64)
    return (cnt + 1) * U23 * mag


# the layout-1 cases of tests/test_gpu_train_conv_kernels_numerics.py's test_roi_pool_backward (one map): C 8, 1, 12 and 40, the
# poolings 7 x 7, 1 x 1, 3 x 5 and 32 x 32, as (C, H, W, PH, PW, N)
GATHER_CASES = tuple(dict.fromkeys(c[:6] for c in K.ROI_CASES if c[6] <= 1))
ROI_STRIDES = ((5, 0), (20, 0), (20, 3), (7, 0))   # (roi_stride, the region = which 5 floats of a table row are selected)


def gather_inputs(case, rule):
    """-> feat [C, H, W], rois [N, 5], g [N, C, PP], argmax [N, C, PP] (the forward's rule restated: K.window_argmax)"""
    C, H, W, PH, PW, N = case
    feat, rois, g = K.roi_inputs(C, H, W, PH, PW, N, 0)
    return feat[0], rois, g, K.window_argmax(feat[0], rois, PH, PW, K.ROI_SCALE, rule)


def roi_table(rois5, stride, region, fill=np.nan):
    """[N, 5] -> the [N * stride] table whose row n holds rois5[n] at floats [5 * region, 5 * region + 5) and `fill` elsewhere"""
    r = np.asarray(rois5, F32)
    t = np.full((len(r), stride), fill, F32)
    t[:, 5 * region:5 * region + 5] = r
    return t.reshape(-1)


def untouched_cells(argmaxes, C, H, W):
    """bool [C, H * W]: the cells no term of any of the given argmax tensors reaches"""
    hit = np.zeros((C, H * W), bool)
    for am in argmaxes:
        am = np.asarray(am).astype(np.int64)
        for c in range(C):
            v = am[:, c, :].reshape(-1)
            hit[c, v[v >= 0]] = True
    return ~hit


NAN_PAYLOAD = np.array([0x7FC12345], np.uint32).view(F32)[0]


def start_map(case, argmaxes, seed=0):
    """-> (a map of random values the chain starts from, the cells made special): where the argmaxes leave two cells alone, one holds
    -0.0 and one a NaN with a payload"""
    C, H, W = case[:3]
    rng = np.random.default_rng(list(case) + [seed, 41])
    m = R.draw(rng, (C, H * W))
    free = np.argwhere(untouched_cells(argmaxes, C, H, W))
    special = []
    if len(free) >= 2:
        (c0, i0), (c1, i1) = free[0], free[-1]
        m[c0, i0], m[c1, i1] = F32(-0.0), NAN_PAYLOAD
        special = [(int(c0), int(i0)), (int(c1), int(i1))]
    return m.reshape(C, H, W), special


def third_argmax(am):
    """a third argmax tensor for the three-call chain: the rows in reverse order (the same cells, other rows feed them)"""
    return np.ascontiguousarray(np.asarray(am)[::-1])


# ---- int_to_float -------------------------------------------------------------------------------------------------------------------
I2F_N = (1, 255, 256, 257, 4099)
I2F_SPECIAL = (-1, 0, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, -2 ** 31, 2 ** 31 - 1)


def i2f_inputs(n):
    """-> a list of int32 [n] arrays.  n = 1: each special value alone.  Otherwise one array of random ints of every magnitude with the
    special values at every third place and, cycled, in the last seven (whatever the tail of a launch, it holds all of them)"""
    sp = np.array(I2F_SPECIAL, np.int64)
    if n == 1:
        return [np.array([v], np.int64).astype(np.int32) for v in sp]
    rng = np.random.default_rng([n, 43])
    v = rng.integers(-2 ** 31, 2 ** 31, n) >> rng.integers(0, 31, n)
    v[::3] = sp[np.arange(len(v[::3])) % 7]
    v[n - 7:] = sp
    return [v.astype(np.int32)]


# ---- linear_dgrad_c8 as the tower backward launches it ------------------------------------------------------------------------------
# the mix weight is packed for Kfull = c5 + c4 + c3 columns and the launch passes K = c5: chunks < K / 8 of the pack are conv5's.  ONE
# launch covers the (PP - 1) * Mp + B rows from the first segment's first row to the last segment's last; row seg * Mp + m is valid for
# m < B, stale otherwise.
DG_KFULL, DG_K, DG_MP = 48 + 24 + 24, 48, 8
DG_CASES = tuple((N, PP, B) for N in (24, 5) for PP in (4, 1) for B in (3, 8))


def dgrad_inputs(N, PP, B):
    """-> g [PP * Mp, N] integers in [-2, 2] (every row drawn: the caller poisons the stale ones), w [N, Kfull] integers, valid [PP * Mp]"""
    rng = np.random.default_rng([N, PP, B, 47])
    g = rng.integers(-2, 3, (PP * DG_MP, N)).astype(F32)
    w = rng.integers(-2, 3, (N, DG_KFULL)).astype(F32)
    valid = (np.arange(PP * DG_MP) % DG_MP) < B
    return g, w, valid


def lin_pack_zero_pad(w):
    """R.lin_pack of w [N, K] with the pad k lanes of the rows n < N +0.0 (what pack_linear_weights writes) and the rows n >= N NaN"""
    N, Kk = w.shape
    out = R.lin_pack(w, 1, fill=SENT_F)
    pad = ~R.lin_valid(Kk, N, 1)
    pad[:, N:, :] = False
    out[pad] = 0.0
    return out
