"""Every launch form behind resnet.hip's convolution dispatcher (rn_conv) against a float64 convolution computed on the host.

The forms are reached one at a time through mpn_debug_conv_form (debug flavour only): the weights are packed by rn_pack into a scratch graph,
the input is laid out as C8I with finite garbage in its pad channel planes and pad rows, and the output lands in a channel slice of a wider
tensor pre-filled with a sentinel NaN.  Every case asserts the form that actually ran (mpn_debug_conv_last_form), so an eligibility rule
cannot quietly send a case to another kernel.  Four tiers:
  * exact: small-integer operands with sum |x w| + |b| + |res| <= 256, so every partial sum is exact in fp32 and the result exact in bf16
    (F(2x2,3x3) Winograd too): each form equals the float64 result bit for bit; blocks outside the op's channel range keep the sentinel;
    what a form writes into its pad channels and pad rows is pinned (PAD_ROWS);
  * accuracy: He-scaled weights on non-negative, mixed-sign and wide-range activations; e = |y - y64| / (sum |x w| + |b| + |res|) against
    the oracle's sequential fp32 chain (O.conv2d_rect), within ACC_FACTOR of it (bf16: on bf16 operands, plus one bf16 rounding);
  * edge: +-inf, NaN, large and subnormal values on map borders and in the first / last channel: every output's class (NaN, +inf, -inf,
    finite) matches an elementwise float64 sum; ReLU(NaN) is pinned per form (RELU_NAN, the rule include/mpn.h states);
  * invariance: per-ROI layers give a map the same bits whatever batch it shares (prefix, slice, permutation, both sides of the bf16
    32 768-pixel threshold, the mosaic after a larger batch); every form is bit-identical run to run; split-K agrees with the unsplit form.

Measured on the MI355X (accuracy tier, worst of the three data sets, e over the oracle chain's e): conv2d_c8i_kernel<1..4> 1.15-1.30,
pf 1.04-1.28, split-K 0.21-0.66, pointwise GEMM (row-invariant) 1.21, 1x1-map GEMM 1.15, im2col GEMM 0.29, Winograd mosaic 0.69-1.09;
bf16 (beyond the final rounding): small kernel / split-K 0.00-0.01, B-direct 0.02-0.21, LDS-DMA 0.00.
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KNOB_DEFAULTS = dict(fp32_pf=1, bf16_dma=1, bf16_dma_tn=0, bf16_bdir=1, bf16_bdir_ver=1, bf16_split_target=256, split_max_tiles=192,
                     graph_fuse=511, roi_invariant=1)
SENT32, SENT16 = 0x7FA5A5A5, 0x7FA5
NOSPLIT = dict(bf16_split_target=0)

# form ids (mpn_debug_conv_last_form): enum ConvForm in graph_internal.h
KC1, KC2, KC3, KC4, PF, MOSAIC, IM2COL, GEMM_FC, GEMM_DIRECT, GEMM_RI = 1, 2, 3, 4, 5, 10, 11, 12, 13, 14
BDIR, DMA_256x128, DMA_128x256, DMA_256x256, B_KP1, B_KP2 = 20, 21, 22, 23, 26, 27
DMA_W8, BDIR8 = 29, 38  # debug-flavour experiments: the 8-wave LDS-DMA shape, the 256-cout B-direct kernel
SPLIT = 0x100
GEMM_FORMS = (IM2COL, GEMM_FC, GEMM_DIRECT, GEMM_RI)
# what a form leaves in the rows from P up to the pitch of its output planes: every form, the GEMM ones included, stores only rows < P
# (measured: the sentinel survives); channels past Cout inside the GEMM's 128-channel panel are written finite
PAD_ROWS = {}
# ReLU(NaN) per form: the fp32 convolution kernels and the GEMM keep NaN (t < 0 ? 0 : t); the Winograd mosaic and every bf16 form give 0
RELU_NAN = {MOSAIC: 0.0}
for _f in (BDIR, DMA_256x128, DMA_128x256, DMA_256x256, B_KP1, B_KP2, DMA_W8, BDIR8):
    RELU_NAN[_f] = RELU_NAN[_f | SPLIT] = 0.0


def _s(B, Cin, H, W, Cout, KH=3, KW=None, sh=1, sw=None, ph=None, pw=None):
    KW = KH if KW is None else KW
    sw = sh if sw is None else sw
    ph = KH // 2 if ph is None else ph
    pw = (KW // 2 if KW == KH else 0) if pw is None else pw
    return dict(B=B, Cin=Cin, H=H, W=W, Cout=Cout, KH=KH, KW=KW, sh=sh, sw=sw, ph=ph, pw=pw)


# name: (expected form, dtype bf16, knobs, shape, flags).  flags: per_roi, gemm (allow_gemm), mosaic (max_rois), res (residual allowed),
# norelu (a norelu channel range allowed: the GEMM / mosaic / im2col forms take only layers without one)
CASES = {
    # fp32, conv2d_c8i_kernel<KC> (KC = 8-channel chunks per stage: nch % 4 / 3 / 2)
    "kc1_cin5": (KC1, 0, NOSPLIT, _s(2, 5, 7, 7, 65)),
    "kc1_cin3_7x7s2": (KC1, 0, NOSPLIT, _s(1, 3, 17, 17, 64, 7, sh=2, ph=3, pw=3)),
    "kc1_cin33_1x1p1": (KC1, 0, NOSPLIT, _s(2, 33, 8, 8, 8, 1, ph=1, pw=1)),
    "kc2_cin9_1x7": (KC2, 0, NOSPLIT, _s(3, 9, 8, 8, 60, 1, 7, ph=0, pw=3)),
    "kc2_cin16_5x5": (KC2, 0, NOSPLIT, _s(1, 16, 17, 17, 8, 5, ph=2, pw=2)),
    "kc3_cin24_3x3s2p0": (KC3, 0, NOSPLIT, _s(2, 24, 17, 17, 129, 3, sh=2, ph=0, pw=0)),
    "kc3_cin65_7x1": (KC3, 0, NOSPLIT, _s(3, 65, 7, 7, 72, 7, 1, ph=3, pw=0)),
    "kc4_cin32_3x3p2": (KC4, 0, dict(fp32_pf=0, bf16_split_target=0), _s(2, 32, 8, 8, 127, 3, ph=2, pw=2)),
    "kc4_cin31_1x1s2": (KC4, 0, dict(fp32_pf=0, bf16_split_target=0), _s(5, 31, 8, 8, 1, 1, sh=2, ph=0, pw=0)),
    "pf_cin64": (PF, 0, NOSPLIT, _s(5, 64, 7, 7, 200)),
    "pf_cin2048_1x1s2": (PF, 0, NOSPLIT, _s(2, 2048, 7, 7, 257, 1, sh=2, ph=0, pw=0)),
    "pf_cin32_3x1": (PF, 0, NOSPLIT, _s(1, 32, 97, 131, 5, 3, 1, ph=1, pw=0)),
    # fp32 split-K + conv_splitk_finalize_kernel (the default dispatch of small layers)
    "split_pf": (PF | SPLIT, 0, {}, _s(2, 64, 8, 8, 128)),
    "split_kc1": (KC1 | SPLIT, 0, {}, _s(1, 33, 7, 7, 5)),
    "split_kc3_1x3": (KC3 | SPLIT, 0, {}, _s(2, 48, 7, 7, 64, 1, 3, ph=0, pw=1)),
    "split_kc2_11x11s4": (KC2 | SPLIT, 0, {}, _s(1, 16, 97, 131, 64, 11, sh=4, ph=2, pw=2)),
    "split_kc4": (KC4 | SPLIT, 0, dict(fp32_pf=0), _s(1, 65 - 1, 2, 2, 192, 3)),
    # the GEMM forms (dense.hip linear_c8) and the Winograd mosaic
    "gemm_direct_res": (GEMM_DIRECT, 0, {}, _s(1, 64, 128, 128, 128, 1), dict(gemm=1)),
    "gemm_ri2_res": (GEMM_RI, 0, {}, _s(5, 64, 7, 7, 65, 1), dict(gemm=1, per_roi=1)),
    "gemm_fc_1x1maps": (GEMM_FC, 0, {}, _s(129, 128, 1, 1, 257, 1), dict(gemm=1, res=0)),
    "im2col_11x11s4": (IM2COL, 0, {}, _s(1, 3, 97, 131, 64, 11, sh=4, ph=2, pw=2), dict(gemm=1, res=0)),
    "im2col_7x7s2": (IM2COL, 0, {}, _s(1, 3, 17, 17, 5, 7, sh=2, ph=3, pw=3), dict(gemm=1, res=0)),
    "mosaic_7x7_roi": (MOSAIC, 0, {}, _s(20, 64, 7, 7, 72), dict(per_roi=1, mosaic=40, res=0)),
    "mosaic_8x8": (MOSAIC, 0, {}, _s(7, 16, 8, 8, 8), dict(mosaic=16, res=0)),
    # 8x8 maps (odd mosaic pitch) in a per-ROI layer: the tile phase would depend on the batch index -> the generic kernel
    "mosaic_8x8_roi_generic": (PF, 0, {}, _s(7, 32, 8, 8, 64), dict(per_roi=1, mosaic=16, res=0)),
    # bf16: conv2d_c8i_bf16_kernel<KP> (KP = 16-channel pairs per stage: nch2 % 4), unsplit and split-K
    "b_kp1_cin40": (B_KP1, 1, NOSPLIT, _s(2, 40, 8, 8, 65)),
    "b_kp1_cin3_7x7s2": (B_KP1, 1, NOSPLIT, _s(1, 3, 17, 17, 64, 7, sh=2, ph=3, pw=3)),
    "b_kp2_cin31_s2": (B_KP2, 1, NOSPLIT, _s(1, 31, 17, 17, 127, 3, sh=2)),
    "b_kp2_cin64_5x5": (B_KP2, 1, NOSPLIT, _s(3, 64, 7, 7, 16, 5)),
    "b_split_kp2": (B_KP2 | SPLIT, 1, {}, _s(2, 64, 8, 8, 128)),
    "b_split_kp1_5x5": (B_KP1 | SPLIT, 1, {}, _s(1, 9, 17, 17, 48, 5)),
    # bf16 large-layer kernels forced onto small maps (bf16_dma = 2: every eligible layer)
    "b_bdir_1x3_c200": (BDIR, 1, dict(bf16_dma=2, bf16_bdir=2), _s(3, 64, 8, 8, 200, 1, 3, ph=0, pw=1)),
    "b_bdir_3x1_c60": (BDIR, 1, dict(bf16_dma=2, bf16_bdir=2), _s(2, 32, 7, 7, 60, 3, 1, ph=1, pw=0)),
    "b_bdir_c257": (BDIR, 1, dict(bf16_dma=2, bf16_bdir=2), _s(2, 64, 7, 7, 257)),
    "b_bdir_c192_s2": (BDIR, 1, dict(bf16_dma=2, bf16_bdir=2), _s(1, 2048, 7, 7, 192, 3, sh=2)),
    "b_dma_256x128": (DMA_256x128, 1, dict(bf16_dma=2, bf16_bdir=0, bf16_dma_tn=128), _s(3, 64, 17, 17, 256, 1, sh=2, ph=0, pw=0)),
    "b_dma_128x256": (DMA_128x256, 1, dict(bf16_dma=2, bf16_bdir=0, bf16_dma_tn=1256), _s(2, 32, 8, 8, 129)),
    "b_dma_256x256": (DMA_256x256, 1, dict(bf16_dma=2, bf16_bdir=0, bf16_dma_tn=256), _s(2, 2048, 7, 7, 512, 1)),
    "b_dma_256x256_7x7s2": (DMA_256x256, 1, dict(bf16_dma=2, bf16_bdir=0, bf16_dma_tn=256), _s(1, 64, 17, 17, 256, 7, sh=2, ph=3, pw=3)),
    # debug-flavour experiments (bit-identical to the product forms): cout count a multiple of 256; ragged 256-cout and pixel tiles
    "b_dma_w8": (DMA_W8, 1, dict(bf16_dma=2, bf16_bdir=0, bf16_dma_tn=2256), _s(2, 64, 8, 8, 256, 1)),
    "b_bdir8_c257": (BDIR8, 1, dict(bf16_dma=2, bf16_bdir=2, bf16_bdir_ver=8), _s(2, 64, 7, 7, 257)),
    # the default dispatch across the 32 768-pixel threshold of a per-ROI layer (7x7 maps: B = 668 -> 32 732 px, B = 669 -> 32 781 px)
    "b_roi_668_small": (B_KP2, 1, {}, _s(668, 64, 7, 7, 192), dict(per_roi=1)),
    "b_roi_669_bdir": (BDIR, 1, {}, _s(669, 64, 7, 7, 192), dict(per_roi=1)),
    "b_roi_669_dma": (None, 1, {}, _s(669, 64, 7, 7, 256, 1), dict(per_roi=1)),
}
BIG = {"b_roi_668_small", "b_roi_669_bdir", "b_roi_669_dma", "gemm_direct_res"}


def _flags(name):
    c = CASES[name]
    f = dict(per_roi=0, gemm=0, mosaic=0, res=1, norelu=1)
    if c[0] in GEMM_FORMS or c[0] == MOSAIC:
        f["norelu"] = 0
    f.update(c[4] if len(c) > 4 else {})
    return f


def _dims(s):
    OH = (s["H"] + 2 * s["ph"] - s["KH"]) // s["sh"] + 1
    OW = (s["W"] + 2 * s["pw"] - s["KW"]) // s["sw"] + 1
    return OH, OW


def _dma_pick(P, Cout):
    """rn_conv's LDS-DMA tile shape for a layer (block rounds over 256 CUs x work per block; ties to the earlier shape)"""
    CoutP = (Cout + 127) // 128 * 128
    best, cost0 = None, None
    for f, tm, tn in ((DMA_256x128, 256, 128), (DMA_128x256, 128, 256), (DMA_256x256, 256, 256)):
        if tm == 256 and CoutP % 256:
            continue
        nb = (P + tn - 1) // tn * (CoutP // tm)
        cost = (nb + 255) // 256 * tm * tn
        if best is None or cost < cost0:
            best, cost0 = f, cost
    return best


def _expected_form(name):
    f, s = CASES[name][0], CASES[name][3]
    if f is None:
        OH, OW = _dims(s)
        return _dma_pick(s["B"] * OH * OW, s["Cout"])
    return f


@functools.lru_cache(maxsize=None)
def _dbg():
    from multipathnet_amd import _lib
    lib = _lib.load("debug")
    vp, i = C.c_void_p, C.c_int
    lib.mpn_debug_conv_form.argtypes = [vp, i, i, i, vp, i, i, i, i, i, i, i, vp, vp, i, i, i, i, i, i, i, i, i, C.POINTER(C.c_int), i, i,
                                        C.c_float, vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    lib.mpn_debug_conv_last_form.restype = i
    return lib


@contextlib.contextmanager
def _knobs(lib, **kv):
    for k, v in kv.items():
        getattr(lib, "mpn_debug_set_" + k)(v)
    try:
        yield
    finally:
        for k in kv:
            getattr(lib, "mpn_debug_set_" + k)(KNOB_DEFAULTS[k])


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def bf16(a):
    """RNE to bf16 and back (NaN / inf kept)"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def run(name, x, w, b=None, res=None, relu=0, norelu=(0, 0), out_c=None, c_off=0, pad_fill=3.0, reps=None, raw=False, knobs=None):
    """one rn_conv call of case `name`; returns y [B, Cout, OH, OW] float32 (and the raw output buffer, its geometry)"""
    from multipathnet_amd import _lib
    form, isbf, kn, s = CASES[name][:4]
    fl = _flags(name)
    lib = _dbg()
    dev = torch.device("cuda", 0)
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    OH, OW = _dims(s)
    reps = list(reps or [B])
    Bl = reps[-1]
    out_c = out_c or c_off + Cout
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    wd = torch.from_numpy(np.ascontiguousarray(w, np.float32)).to(dev)
    bd = torch.from_numpy(np.ascontiguousarray(b, np.float32)).to(dev) if b is not None else None
    rd = torch.from_numpy(np.ascontiguousarray(res, np.float32)).to(dev) if res is not None else None
    y = torch.empty((Bl, Cout, OH, OW), dtype=torch.float32, device=dev)
    pitch = (Bl * OH * OW + 127) // 128 * 128
    nblk = max((out_c + 127) // 128 * 128, c_off + (Cout + 127) // 128 * 128) // 8
    esz = 2 if isbf else 4
    rawd = torch.empty(nblk * pitch * 8 * esz, dtype=torch.uint8, device=dev) if raw else None
    nb = (C.c_int * len(reps))(*reps)
    form_out = C.c_int(-1)
    rb = C.c_size_t(0)
    torch.cuda.synchronize()
    with _knobs(lib, **dict(kn, **(knobs or {}))):
        rc = lib.mpn_debug_conv_form(_ptr(xd), Cin, H, W, _ptr(wd), Cout, s["KH"], s["KW"], s["sh"], s["sw"], s["ph"], s["pw"], _ptr(bd), _ptr(rd),
                                     int(relu), norelu[0], norelu[1], isbf, fl["per_roi"], fl["gemm"], fl["mosaic"], fl["mosaic"], len(reps), nb,
                                     out_c, c_off, float(pad_fill), _ptr(y), _ptr(rawd), rawd.numel() if raw else 0, C.byref(rb), C.byref(form_out))
    if rc != 0:
        raise _lib.MpnError("mpn_debug_conv_form(%s) failed (%d): %s" % (name, rc, lib.mpn_last_error().decode()))
    assert lib.mpn_debug_conv_last_form() == form_out.value
    if knobs is None:
        assert form_out.value == _expected_form(name), "%s ran form %#x, meant %#x" % (name, form_out.value, _expected_form(name))
    yh = y.cpu().numpy()
    if not raw:
        return yh
    assert rb.value == rawd.numel()
    r = rawd.cpu().numpy().view(np.uint16 if isbf else np.uint32).reshape(nblk, pitch, 8)
    return yh, r, form_out.value


# ---------------------------------------------------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------------------------------------------------
def ref64(name, x, w, b=None, res=None, relu=0, norelu=(0, 0), absolute=False):
    s = CASES[name][3]
    xt, wt = torch.from_numpy(np.asarray(x, np.float64)), torch.from_numpy(np.asarray(w, np.float64))
    if absolute:
        xt, wt = xt.abs(), wt.abs()
    bt = torch.from_numpy(np.asarray(b, np.float64)) if b is not None else None
    if absolute and bt is not None:
        bt = bt.abs()
    y = torch.nn.functional.conv2d(torch.nn.functional.pad(xt, (s["pw"], s["pw"], s["ph"], s["ph"])), wt, bt, stride=(s["sh"], s["sw"])).numpy()
    if res is not None:
        y = y + (np.abs(res) if absolute else res)
    if relu and not absolute:
        y = _relu_ref(y, norelu)
    return y


def _relu_ref(y, norelu, nan_to=None):
    y = y.copy()
    ch = np.ones(y.shape[1], bool)
    ch[norelu[0]:norelu[1]] = False
    v = y[:, ch]
    m = v < 0
    if nan_to is not None:
        m |= np.isnan(v)
    v[m] = 0.0 if nan_to is None else np.where(np.isnan(v[m]), nan_to, 0.0)
    y[:, ch] = v
    return y


def ref_elementwise(name, x, w, b=None, res=None):
    """float64 as an explicit sum of elementwise products (0 * inf = NaN, as the kernels compute it; no BLAS)"""
    s = CASES[name][3]
    xt = torch.nn.functional.pad(torch.from_numpy(np.asarray(x, np.float64)), (s["pw"], s["pw"], s["ph"], s["ph"]))
    B = x.shape[0]
    Cout = w.shape[0]
    OH, OW = _dims(s)
    cols = torch.nn.functional.unfold(xt, (s["KH"], s["KW"]), stride=(s["sh"], s["sw"])).numpy()  # [B, Cin*KK, L]
    wf = np.asarray(w, np.float64).reshape(Cout, -1)
    y = np.zeros((B, Cout, OH * OW))
    for bi in range(B):
        for c0 in range(0, Cout, 16):
            y[bi, c0:c0 + 16] = (wf[c0:c0 + 16, :, None] * cols[bi][None, :, :]).sum(1)  # [couts, K, L] products, summed over K
    y = y.reshape(B, Cout, OH, OW)
    if b is not None:
        y = y + np.asarray(b, np.float64)[None, :, None, None]
    if res is not None:
        y = y + res
    return y


# ---------------------------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------------------------
def exact_operands(name, seed):
    """small integers: each output channel has at most 60 non-zero weights of |w| <= 2 against |x| <= 2, |b| <= 8, |res| <= 8"""
    s = CASES[name][3]
    rng = np.random.default_rng(seed)
    B, Cin, H, W, Cout, KH, KW = (s[k] for k in ("B", "Cin", "H", "W", "Cout", "KH", "KW"))
    x = rng.integers(-2, 3, (B, Cin, H, W)).astype(np.float32)
    K = Cin * KH * KW
    w = np.zeros((Cout, K), np.float32)
    nz = min(K, 60)
    for co in range(Cout):
        idx = rng.choice(K, nz, replace=False)
        idx[:2] = [0, K - 1][:nz]  # the first and the last (channel, tap) always take part
        w[co, idx] = rng.integers(-2, 3, nz)
    w = w.reshape(Cout, Cin, KH, KW)
    b = rng.integers(-8, 9, Cout).astype(np.float32)
    OH, OW = _dims(s)
    res = rng.integers(-8, 9, (B, Cout, OH, OW)).astype(np.float32)
    return x, w, b, res


def _norelu_ranges(name, Cout):
    """norelu variants: empty, the first block, one in the middle, the tail block (8 channels fp32, 16 bf16)"""
    g = 16 if CASES[name][1] else 8
    nb = (Cout + g - 1) // g
    out = [(0, 0)]
    if not _flags(name)["norelu"] or nb < 2:
        return out
    out.append((0, g))
    if nb >= 3:
        out.append(((nb // 2) * g, (nb // 2 + 1) * g))
    out.append(((nb - 1) * g, nb * g))
    return out


def _epilogues(name, Cout):
    """(bias, res, relu, norelu) combinations run in the exact tier"""
    fl = _flags(name)
    eps = [(True, False, 0, (0, 0)), (False, False, 1, (0, 0))]
    if fl["res"]:
        eps.append((True, True, 1, (0, 0)))
    for nr in _norelu_ranges(name, Cout)[1:]:
        eps.append((True, bool(fl["res"]), 1, nr))
    return eps


def _placement(name, Cout):
    """(out_c, c_off) of the wider DepthConcat tensor: a block of other channels on both sides unless the form writes whole 128-channel
    panels (the graph gives those forms only tensors they own)"""
    if CASES[name][0] in GEMM_FORMS:
        return Cout, 0
    g = 16 if CASES[name][1] else 8
    c_off = 2 * g
    return c_off + (Cout + g - 1) // g * g + g, c_off


EXACT = [n for n in CASES if n not in BIG] + ["gemm_direct_res"]


@pytest.mark.parametrize("name", EXACT)
def test_exact(name):
    """bit-exact against float64 for every epilogue; sentinel outside the op's blocks; pad channels / rows as PAD_ROWS states"""
    form, isbf, _, s = CASES[name][:4]
    Cout = s["Cout"]
    x, w, b, res = exact_operands(name, 11 + len(name))
    OH, OW = _dims(s)
    P = s["B"] * OH * OW
    Cb = (Cout + 7) // 8
    out_c, c_off = _placement(name, Cout)
    sent = SENT16 if isbf else SENT32
    for i, (hb, hr, relu, nr) in enumerate(_epilogues(name, Cout)):
        bb, rr = (b if hb else None), (res if hr else None)
        y, raw, f = run(name, x, w, bb, rr, relu, nr, out_c=out_c, c_off=c_off, pad_fill=(3.0, -1.0e4, 0.5)[i % 3], raw=True)
        y64 = ref64(name, x, w, bb, rr, relu, nr)
        assert np.array_equal(y, y64), "%s epilogue %d: %d outputs differ, max |d| %g" % (name, i, int((y != y64).sum()), np.abs(y - y64).max())
        b0, b1 = c_off // 8, c_off // 8 + Cb
        if f in GEMM_FORMS:
            b1w = c_off // 8 + (Cout + 127) // 128 * 16
            assert np.isfinite(raw[b1:b1w, :P].view(np.float32)).all()   # channels past Cout in the panel: finite
        else:
            b1w = b1
        outside = np.concatenate([raw[:b0].ravel(), raw[b1w:].ravel()])
        assert (outside == sent).all(), "%s: %d elements outside the op's channel blocks were written" % (name, int((outside != sent).sum()))
        own = raw[b0:b1]
        vals = (own.astype(np.uint32) << np.uint32(16)).view(np.float32) if isbf else own.view(np.float32)
        assert np.isfinite(vals[-1, :P, Cout - (Cb - 1) * 8:]).all(), "%s: pad channels of the last block must be finite" % name
        if PAD_ROWS.get(f) == "finite":
            assert np.isfinite(vals[:, P:]).all(), "%s: pad rows" % name
        else:
            assert (own[:, P:] == sent).all(), "%s: the form wrote pad rows" % name


# ---------------------------------------------------------------------------------------------------------------------------------------
# accuracy
# ---------------------------------------------------------------------------------------------------------------------------------------
# largest e(form) / e(oracle fp32 chain) allowed; bf16: of the fp32 part, after one bf16 rounding (2^-8 |y|) is taken off
ACC_FACTOR = {"fp32": 1.5, MOSAIC: 2.0, "bf16": 1.5}
ACC = ["kc1_cin5", "kc2_cin16_5x5", "kc3_cin65_7x1", "kc4_cin32_3x3p2", "pf_cin64", "pf_cin2048_1x1s2", "split_pf", "split_kc2_11x11s4",
       "split_kc3_1x3", "gemm_ri2_res", "gemm_fc_1x1maps", "im2col_11x11s4", "mosaic_7x7_roi", "mosaic_8x8", "b_kp1_cin40", "b_kp2_cin31_s2",
       "b_split_kp2", "b_split_kp1_5x5", "b_bdir_1x3_c200", "b_bdir_c192_s2", "b_dma_256x128", "b_dma_128x256", "b_dma_256x256",
       "b_roi_669_bdir"]
MEASURED = {}


def acc_operands(name, kind, seed):
    s = CASES[name][3]
    rng = np.random.default_rng(seed)
    B, Cin, H, W, Cout, KH, KW = (s[k] for k in ("B", "Cin", "H", "W", "Cout", "KH", "KW"))
    x = rng.standard_normal((B, Cin, H, W)).astype(np.float32)
    if kind == "nonneg":
        x = np.abs(x)
    elif kind == "wide":
        x = (x * np.exp2(rng.uniform(-12, 12, x.shape))).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, KH, KW)) * np.sqrt(2.0 / (Cin * KH * KW))).astype(np.float32)
    b = (rng.standard_normal(Cout) * 0.1).astype(np.float32)
    OH, OW = _dims(s)
    res = rng.standard_normal((B, Cout, OH, OW)).astype(np.float32) if _flags(name)["res"] else None
    if CASES[name][1]:
        x, w, res = bf16(x), bf16(w), (bf16(res) if res is not None else None)
    return x, w, b, res


@pytest.mark.parametrize("kind", ["nonneg", "mixed", "wide"])
@pytest.mark.parametrize("name", ACC)
def test_accuracy(name, kind, O):
    form, isbf, _, s = CASES[name][:4]
    x, w, b, res = acc_operands(name, kind, 101 + len(name))
    y = run(name, x, w, b, res)
    y64 = ref64(name, x, w, b, res)
    den = ref64(name, x, w, b, res, absolute=True)
    den = np.maximum(den, np.finfo(np.float32).tiny)
    yo = O.conv2d_rect(x, w, b, s["sh"], s["sw"], s["ph"], s["pw"], False).astype(np.float64)
    if res is not None:
        yo = (yo.astype(np.float32) + res).astype(np.float64)
    e_orc = (np.abs(yo - y64) / den).max()
    e_orc = max(e_orc, 2.0 ** -24)
    if isbf:
        e = (np.maximum(np.abs(y - y64) - 2.0 ** -8 * np.abs(y64), 0) / den).max()
        fac = ACC_FACTOR["bf16"]
    else:
        e = (np.abs(y - y64) / den).max()
        fac = ACC_FACTOR[MOSAIC] if form == MOSAIC else ACC_FACTOR["fp32"]
    MEASURED[(name, kind)] = e / e_orc
    print("ACC %s %s ratio %.3f (e %.3g, oracle %.3g)" % (name, kind, e / e_orc, e, e_orc))
    assert e <= fac * e_orc, "%s/%s: error %.3g is %.2fx the oracle chain's %.3g" % (name, kind, e, e / e_orc, e_orc)


# ---------------------------------------------------------------------------------------------------------------------------------------
# edge values
# ---------------------------------------------------------------------------------------------------------------------------------------
EDGE = ["kc1_cin5", "kc2_cin9_1x7", "kc3_cin24_3x3s2p0", "kc4_cin32_3x3p2", "pf_cin64", "split_pf", "split_kc1", "gemm_ri2_res",
        "gemm_fc_1x1maps", "im2col_7x7s2", "b_kp1_cin40", "b_kp2_cin64_5x5", "b_split_kp2", "b_split_kp1_5x5", "b_bdir_1x3_c200",
        "b_bdir_3x1_c60", "b_dma_256x128", "b_dma_128x256", "b_dma_256x256_7x7s2", "b_dma_w8", "b_bdir8_c257"]


def edge_operands(name, seed):
    s = CASES[name][3]
    rng = np.random.default_rng(seed)
    B, Cin, H, W = (s[k] for k in ("B", "Cin", "H", "W"))
    x, w, b, res = acc_operands(name, "mixed", seed)
    # on map borders (next to the padding), in the first and the last channel
    spots = [(0, 0, 0, 0, np.nan), (1, Cin - 1, H - 1, W - 1, np.inf), (2, 0, 0, W - 1, -np.inf), (-1, Cin - 1, H - 1, 0, np.nan),
             (3, Cin // 2, H // 2, W // 2, 1.0e30), (-2, Cin // 2, 0, W // 2, -1.0e30), (4, Cin - 1, 0, W // 2, 1.0e-40),
             (-3, 0, H // 2, 0, -3.0e-39)]
    for bi, c, yy, xx, v in spots:  # one map per value where the batch allows it (1x1 maps)
        x[bi % B, c, yy, xx] = v
    # subnormal and large weights at the first and the last (channel, tap)
    w[0, 0, 0, 0] = 1.0e-40
    w[-1, -1, -1, -1] = 1.0e20
    if CASES[name][1]:
        x, w = bf16(x), bf16(w)
    return x, w, b, res


def _cls(a):
    return np.where(np.isnan(a), 0, np.where(a == np.inf, 1, np.where(a == -np.inf, 2, 3)))


@pytest.mark.parametrize("name", EDGE)
def test_edge_classes(name):
    """every output's class matches the elementwise float64 sum, without ReLU, inside a norelu range and (per RELU_NAN) with ReLU"""
    form = _expected_form(name)
    Cout = CASES[name][3]["Cout"]
    x, w, b, res = edge_operands(name, 7 + len(name))
    y64 = ref_elementwise(name, x, w, b, res)
    assert np.isnan(y64).any() and np.isinf(y64).any() and np.isfinite(y64).any()
    y = run(name, x, w, b, res, relu=0)
    bad = _cls(y) != _cls(y64)
    assert not bad.any(), "%s (no ReLU): %d outputs in the wrong class, e.g. %s vs %s" % (name, int(bad.sum()), y[bad][:4], y64[bad][:4])
    for nr in _norelu_ranges(name, Cout)[-1:] + [(0, 0)]:
        y = run(name, x, w, b, res, relu=1, norelu=nr)
        nan_to = RELU_NAN.get(form)
        yr = _relu_ref(y64, nr, nan_to=nan_to)
        bad = _cls(y) != _cls(yr)
        assert not bad.any(), "%s (ReLU, norelu %s): %d outputs in the wrong class, e.g. %s vs %s" % (name, nr, int(bad.sum()), y[bad][:4], yr[bad][:4])
        ch = np.ones(Cout, bool)
        ch[nr[0]:nr[1]] = False
        if nan_to is not None:
            assert (y[:, ch][np.isnan(y64[:, ch])] == nan_to).all()


def test_edge_mosaic_isolation():
    """the Winograd mosaic spreads a non-finite input over its transform tiles (no elementwise class rule): a map's non-finite values stay
    inside that map, every non-finite float64 output is non-finite, and ReLU(NaN) is 0"""
    name = "mosaic_7x7_roi"
    x, w, b, _ = acc_operands(name, "mixed", 5)
    x0 = x.copy()
    for v, c, yy, xx in ((np.nan, 0, 0, 0), (np.inf, 63, 6, 6), (-np.inf, 5, 3, 0)):
        x[4, c, yy, xx] = v
    y64 = ref_elementwise(name, x[4:5], w, b)
    keep = np.arange(x.shape[0]) != 4
    for relu in (0, 1):
        y = run(name, x, w, b, relu=relu)
        y0 = run(name, x0, w, b, relu=relu)
        assert np.array_equal(y[keep], y0[keep])
        assert np.isfinite(y[keep]).all()
        if relu:
            assert not np.isnan(y).any()  # ReLU(NaN) = 0 (RELU_NAN)
        else:
            assert not np.isfinite(y[4][~np.isfinite(y64[0])]).any()


# ---------------------------------------------------------------------------------------------------------------------------------------
# invariance
# ---------------------------------------------------------------------------------------------------------------------------------------
def _plant(x, b):
    x = x.copy()
    x[b, 0, 0, 0] = np.nan
    x[b, -1, -1, -1] = np.inf
    return x


@pytest.mark.parametrize("planted", [False, True])
@pytest.mark.parametrize("name", ["gemm_ri2_res", "mosaic_7x7_roi", "mosaic_8x8_roi_generic"])
def test_roi_invariance_fp32(name, planted):
    """per-ROI layers: a map's output bits do not depend on the batch (prefix, middle slice, permutation; mosaic: after a larger batch)"""
    x, w, b, res = acc_operands(name, "wide", 3)
    if planted:
        x = _plant(x, 2)
    B = x.shape[0]
    full = run(name, x, w, b, res, relu=1)
    assert np.array_equal(full, run(name, x, w, b, res, relu=1), equal_nan=True)
    k = max(1, B // 3)
    pre = run(name, x[:k], w, b, res[:k] if res is not None else None, relu=1)
    assert np.array_equal(pre, full[:k], equal_nan=True)
    mid = run(name, x[k:2 * k + 1], w, b, res[k:2 * k + 1] if res is not None else None, relu=1)
    assert np.array_equal(mid, full[k:2 * k + 1], equal_nan=True)
    perm = np.random.default_rng(1).permutation(B)
    pp = run(name, x[perm], w, b, res[perm] if res is not None else None, relu=1)
    assert np.array_equal(pp, full[perm], equal_nan=True)
    if _flags(name)["mosaic"] and _expected_form(name) == MOSAIC:
        # B = N, then N / 3 (not a multiple of the mosaic row), then N again, on one graph
        again = run(name, x, w, b, res, relu=1, reps=[B, k, B])
        assert np.array_equal(again, full, equal_nan=True)
        after = run(name, x, w, b, res, relu=1, reps=[B, k])
        assert np.array_equal(after, full[:k], equal_nan=True)


@pytest.mark.parametrize("planted", [False, True])
def test_roi_invariance_bf16_threshold(planted):
    """bf16 per-ROI layer on both sides of the 32 768-pixel threshold: the small kernel (B = 668), the B-direct kernel (B = 669) and the
    LDS-DMA kernel share one K chain: the same bits per map; also for a slice and a permutation"""
    x, w, b, res = acc_operands("b_roi_669_bdir", "mixed", 9)
    if planted:
        x = _plant(x, 600)
    big = run("b_roi_669_bdir", x, w, b, res, relu=1, norelu=(64, 80))
    assert np.array_equal(big, run("b_roi_669_bdir", x, w, b, res, relu=1, norelu=(64, 80)), equal_nan=True)
    small = run("b_roi_668_small", x[:668], w, b, res[:668], relu=1, norelu=(64, 80))
    assert np.array_equal(small, big[:668], equal_nan=True)
    perm = np.random.default_rng(2).permutation(669)
    pp = run("b_roi_669_bdir", x[perm], w, b, res[perm], relu=1, norelu=(64, 80))
    assert np.array_equal(pp, big[perm], equal_nan=True)
    sl = run("b_roi_668_small", x[1:669], w, b, res[1:669], relu=1, norelu=(64, 80))
    assert np.array_equal(sl, big[1:], equal_nan=True)
    # the pointwise layer: LDS-DMA kernel above the threshold, the small kernel below
    x2, w2, b2, res2 = acc_operands("b_roi_669_dma", "mixed", 10)
    if planted:
        x2 = _plant(x2, 600)
    big2 = run("b_roi_669_dma", x2, w2, b2, res2, relu=1)
    small2 = run("b_roi_669_dma", x2[:668], w2, b2, res2[:668], relu=1, knobs={})
    assert np.array_equal(small2, big2[:668], equal_nan=True)
    # and the three LDS-DMA tile shapes and the B-direct kernel on one layer
    for kn in (dict(bf16_bdir=0, bf16_dma_tn=128), dict(bf16_bdir=0, bf16_dma_tn=1256), dict(bf16_bdir=0, bf16_dma_tn=256), dict(bf16_bdir=2)):
        assert np.array_equal(run("b_roi_669_dma", x2, w2, b2, res2, relu=1, knobs=kn), big2, equal_nan=True), kn


RUN_TWICE = ["kc1_cin5", "kc3_cin65_7x1", "pf_cin64", "split_pf", "split_kc2_11x11s4", "split_kc4", "gemm_fc_1x1maps", "im2col_11x11s4",
             "mosaic_8x8", "b_kp1_cin40", "b_split_kp2", "b_split_kp1_5x5", "b_bdir_c257", "b_dma_256x256_7x7s2", "b_dma_128x256", "b_dma_w8", "b_bdir8_c257"]


@pytest.mark.parametrize("name", RUN_TWICE)
def test_deterministic_and_pad_blind(name):
    """bit-identical run after run, and whatever finite garbage the input's pad planes / rows hold"""
    x, w, b, res = acc_operands(name, "wide", 21)
    y1 = run(name, x, w, b, res, relu=1, pad_fill=0.0)
    y2 = run(name, x, w, b, res, relu=1, pad_fill=0.0)
    y3 = run(name, x, w, b, res, relu=1, pad_fill=-7.5e3)
    assert np.array_equal(y1.view(np.uint32), y2.view(np.uint32))
    assert np.array_equal(y1.view(np.uint32), y3.view(np.uint32))


@pytest.mark.parametrize("name", ["split_pf", "split_kc3_1x3", "split_kc2_11x11s4", "b_split_kp2", "b_split_kp1_5x5"])
def test_split_matches_unsplit(name):
    """split-K against the unsplit form of the same kernel: both within the accuracy bound of float64, and close to each other"""
    isbf = CASES[name][1]
    x, w, b, res = acc_operands(name, "mixed", 33)
    ys = run(name, x, w, b, res)
    yu = run(name, x, w, b, res, knobs=NOSPLIT)
    assert _dbg().mpn_debug_conv_last_form() == CASES[name][0] & ~SPLIT
    y64 = ref64(name, x, w, b, res)
    den = np.maximum(ref64(name, x, w, b, res, absolute=True), 1e-30)
    K = x.shape[1] * CASES[name][3]["KH"] * CASES[name][3]["KW"]
    tol = (2.0 ** -8 * np.abs(y64) / den if isbf else 0.0) + 2 * K * 2.0 ** -24
    assert (np.abs(ys - y64) / den <= tol).all() and (np.abs(yu - y64) / den <= tol).all()
