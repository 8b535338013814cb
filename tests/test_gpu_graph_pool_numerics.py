"""The graph executor's pooling, LRN and ROI-pooling kernels (graph_pool.hip), one launch at a time, against float64 restatements.

The kernels are reached through two debug entries (debug flavour only) that run the product's own dispatch on a scratch graph:
mpn_debug_graph_op (graph_parse / graph_dims / graph_run on one max-pool, average-pool or LRN op) and mpn_debug_head_pool
(resnet_head_forward on a head without convolutions: ROI pooling, optionally the max-pool of the pooled map, the closing average).  The
source is laid out as C8I with a finite one-signed pattern (pad_fill * 1..5) in the pad lanes of a ragged last channel block and in the rows
from B*H*W up to the pitch; every output tensor first holds a sentinel NaN.  Every case asserts the id of the kernel that ran (enum PoolKernel).
The references are tests/graph_pool_np.py's, themselves checked against the CPU oracle and PyTorch in tests/test_graph_pool_ref_cpu.py.

Tiers:
  * max-pool (fp32, bf16): equal to the float64 max as values (max is exact; bf16 inputs rounded first); pad_fill exceeds every real value, so
    a read of a pad row or lane would win; the sentinel survives outside the op's channel blocks and in the rows >= B*OH*OW; +-inf / NaN /
    +-0 / all-NaN windows: NaNs ignored, only-NaN -> -inf (include/mpn.h);
  * average pool (fp32, bf16 plain, bf16 small-map LDS kernel; with and without the commuted pool's bias + ReLU): within the derived bound of
    float64 (test_avgpool), and without bias bit-equal to the sequential fp32 emulation of the documented order;
  * LRN: relative error against float64 at most LRN_FACTOR x the oracle chain's on the same inputs; pad lanes of the output exactly 0; the pad
    lanes of the input hold 1e18 .. 5e18, whose squares (1e36 .. 2.5e37) are finite in fp32 and 10^30 times any real square, so a window that
    touched one would shrink the output by a factor of about 1e-23; ragged channel counts run again with 4e19 .. 2e20, whose squares are inf
    in fp32, so the same window would give 0 (alpha > 0) or NaN (alpha = 0: 0 * inf); alpha = 0, k = 1 is the identity bit for bit;
    inf / NaN inputs change only the outputs whose window holds them; the refusals (bf16, even size, size 19);
  * ROI pooling (fp32 per-thread, fp32 rows<4>, bf16 plain, bf16 on the int16-sortable map), both bin rules, roi_stride 5 and 20: equal to
    O.roi_pool bit for bit except between +-0; sorted and plain bf16 kernels against each other on NaN / +-0 features;
  * fused ROI max-pool (with and without range-max tables): the two-step reference bit for bit up to the sign of zero; NaN / +-inf features
    through it and through the fp32 and plain bf16 ROI poolings: NaNs ignored, only-NaN -> -inf;
  * closing average to C8 (fp32, bf16 plain, bf16 LDS): bit-equal to the sequential emulation, within the derived bound, rows >= N untouched;
  * every entry twice: the same bits.

What the NaN / +-0 comparison of the two bf16 ROI-pooling kernels found: the int16 order put a positive NaN above +inf, so the sorted kernel and
the fused max-pool returned NaN for a window holding one where the plain kernel (f > m) ignores it.  Resolved in the encoder
(bf16_sortable_kernel gives a NaN of either sign the code of -inf): both now follow include/mpn.h's rule.  The sign of a zero maximum still
differs (+0 on the sortable map, the zero met first in the plain kernel); that is documented in include/mpn.h and pinned in
test_roi_pool_bf16_sorted_vs_plain_edge_values.

LRN, measured on the MI355X (max relative error over the tensor against float64, in units of 2^-24, 24 cases): device 0.72-4.34, the
oracle's fp32 chain 0.72-3.24 on the same inputs; device / oracle per case 0.80-1.48, worst at C=13, size=17 (1.48), C=96, size=17 (1.34) and
C=5, size=17 (1.32); 11 of the 24 cases give exactly the oracle's error.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import hooks

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_pool_np as R  # noqa: E402

pytestmark = pytest.mark.gpu

LRN_FACTOR = 2.0  # the device powf and a contracted k + a * ssum, over the oracle's fp32 chain

SENT32, SENT16 = 0x7FA5A5A5, 0x7FA5
MPN_EINVAL = -1
# enum PoolKernel (graph_internal.h)
MAX_F32, MAX_BF16, AVG_F32, AVG_BF16, AVG_BF16_SMALL, LRN = 1, 2, 3, 4, 5, 6
ROI_F32, ROI_ROWS4, ROI_BF16, ROI_SORTED = 16, 17, 18, 19
ROIMAX_SORTED, ROIMAX_SORTED_TABLES = 32, 33
GAVG_F32, GAVG_BF16, GAVG_BF16_LDS = 48, 49, 50
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _dbg():
    from multipathnet_amd import _lib
    lib = _lib.load("debug")
    vp, i, f, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    ip = C.POINTER(C.c_int)
    lib.mpn_debug_graph_op.argtypes = [vp, i, i, i, i, C.POINTER(_lib.GraphOp), i, i, i, f, vp, sz, ip, ip, vp, sz, C.POINTER(sz), ip]
    lib.mpn_debug_head_pool.argtypes = [vp, i, i, i, vp, i, i, i, f, i, i, C.POINTER(_lib.GraphOp), f, i, vp, vp, sz, ip, ip, vp, ip, ip]
    return lib


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.device("cuda", 0))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits_up_to_zero_sign(got, ref):
    """bit equality, except that where the reference is a zero any zero will do"""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    z = ref == 0
    return bool((got[z] == 0).all()) and np.array_equal(_bits(got)[~z], _bits(ref)[~z])


def graph_op(x, kind, kh, kw, sh, sw, ph, pw, bf16=0, ceil=0, cin=None, src_c_off=0, out_c=None, c_off=0, pad_fill=3.0, bias=None, relu=0,
             lrn=(0.0, 0.0, 1.0), expect=None, knobs=None):
    """one op through mpn_debug_graph_op.  Returns y [B, cin, OH, OW] float32, the raw output buffer [blocks, pitch, 8] (uint32 / uint16) and the
    kernel id; with a refusal, (rc, message)."""
    from multipathnet_amd import _lib
    lib = _dbg()
    B, Cs, H, W = x.shape
    cin = cin or Cs - src_c_off
    out_c = out_c or c_off + cin
    if kind == 3:
        OH, OW = H, W
    elif kind == 1:
        OH, OW = R.pool_out_size(H, kh, sh, ph, ceil), R.pool_out_size(W, kw, sw, pw, ceil)
    else:
        OH, OW = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    xd = _dev(x)
    bd = _dev(bias) if bias is not None else None
    op = _lib.GraphOp(kind=kind, src=0, dst=1, dst_c_off=c_off, cin=cin, cout=0, kh=kh, kw=kw, sh=sh, sw=sw, ph=ph, pw=pw, relu=int(relu),
                      w=None, b=C.cast(_ptr(bd), _lib.f32p) if bd is not None else None, src_c_off=src_c_off, ceil_mode=int(ceil),
                      lrn_alpha=lrn[0], lrn_beta=lrn[1], lrn_k=lrn[2])
    y = torch.empty((B, cin, max(OH, 1), max(OW, 1)), dtype=torch.float32, device=xd.device)
    pitch = (B * max(OH, 1) * max(OW, 1) + 127) // 128 * 128
    nblk = (out_c + 127) // 128 * 128 // 8
    esz = 2 if bf16 else 4
    rawd = torch.empty(nblk * pitch * 8 * esz, dtype=torch.uint8, device=xd.device)
    oh, ow, kid, rb = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_size_t(0)
    torch.cuda.synchronize()
    with hooks(**(knobs or {})):
        rc = lib.mpn_debug_graph_op(_ptr(xd), B, Cs, H, W, C.byref(op), int(bf16), out_c, c_off, float(pad_fill), _ptr(y), y.numel(), C.byref(oh),
                                    C.byref(ow), _ptr(rawd), rawd.numel(), C.byref(rb), C.byref(kid))
    if rc != 0:
        if expect is None:
            raise _lib.MpnError("mpn_debug_graph_op failed (%d): %s" % (rc, lib.mpn_last_error().decode()))
        return rc, lib.mpn_last_error().decode()
    assert (oh.value, ow.value) == (OH, OW) and rb.value == rawd.numel()
    raw = rawd.cpu().numpy().view(np.uint16 if bf16 else np.uint32).reshape(nblk, pitch, 8)
    return y.cpu().numpy(), raw, kid.value


def check_sentinel(raw, bf16, c_off, cin, rows):
    """the sentinel survives in every channel block outside the op's and, inside them, in the rows >= rows"""
    sent = SENT16 if bf16 else SENT32
    b0, b1 = c_off // 8, c_off // 8 + (cin + 7) // 8
    assert (raw[:b0] == sent).all() and (raw[b1:] == sent).all(), "wrote outside the op's channel blocks"
    assert (raw[b0:b1, rows:] == sent).all(), "wrote rows past B*OH*OW"
    assert not (raw[b0:b1, :rows, :min(cin, 8)] == sent).all()


def head_pool(feat, rois, PH, scale, rule=0, bf16=0, op=None, pad_fill=3.0, Mp=None, knobs=None):
    """resnet_head_forward through mpn_debug_head_pool.  Returns pooled [N, C, PH, PH], the max-pooled tensor (or None), the C8 average as
    uint32 [Cb, Mp, 8], the four kernel ids and the range-max levels built."""
    from multipathnet_amd import _lib
    lib = _dbg()
    Cc, H, W = feat.shape
    N, stride = rois.shape
    Mp = Mp or N + 3
    fd, rd = _dev(feat), _dev(rois)
    pooled = torch.empty((N, Cc, PH, PH), dtype=torch.float32, device=fd.device)
    gop, mp = None, None
    if op is not None:
        k, s, p = op
        OH = R.pool_out_size(PH, k, s, p, 0)
        gop = _lib.GraphOp(kind=1, src=0, dst=1, dst_c_off=0, cin=Cc, cout=0, kh=k, kw=k, sh=s, sw=s, ph=p, pw=p, relu=0, w=None, b=None, src_c_off=0,
                           ceil_mode=0, lrn_alpha=0.0, lrn_beta=0.0, lrn_k=1.0)
        mp = torch.empty((N, Cc, OH, OH), dtype=torch.float32, device=fd.device)
    Cb = (Cc + 7) // 8
    c8 = torch.empty((Cb, Mp, 8), dtype=torch.float32, device=fd.device)
    kids = (C.c_int * 4)()
    oh, ow, lv = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    torch.cuda.synchronize()
    with hooks(**(knobs or {})):
        rc = lib.mpn_debug_head_pool(_ptr(fd), Cc, H, W, _ptr(rd), stride, N, PH, float(scale), int(rule), int(bf16), C.byref(gop) if gop else None,
                                     float(pad_fill), Mp, _ptr(pooled), _ptr(mp), mp.numel() if mp is not None else 0, C.byref(oh), C.byref(ow),
                                     _ptr(c8), kids, C.byref(lv))
    if rc != 0:
        raise _lib.MpnError("mpn_debug_head_pool failed (%d): %s" % (rc, lib.mpn_last_error().decode()))
    if mp is not None:
        assert (oh.value, ow.value) == tuple(mp.shape[2:])
    return pooled.cpu().numpy(), (mp.cpu().numpy() if mp is not None else None), _bits(c8.cpu().numpy()), list(kids), lv.value


def rois_strided(rois5, stride, rng):
    """the [N, 5] table as rows of `stride` floats (the pipeline's 20-float ROI records: the rest is other data)"""
    if stride == 5:
        return rois5
    t = rng.uniform(-1e3, 1e3, (rois5.shape[0], stride)).astype(np.float32)
    t[:, :5] = rois5
    return t


# ---------------------------------------------------------------------------------------------------------------------------------------
# max-pool
# ---------------------------------------------------------------------------------------------------------------------------------------
MAX_C = {0: [8, 20, 24], 1: [16, 24, 48]}


@pytest.mark.parametrize("bf16", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("k,s,p,ceil", R.MAXPOOL_GEOMS)
def test_maxpool(k, s, p, ceil, bf16):
    n = 0
    for mi, (H, W) in enumerate(R.MAXPOOL_MAPS + [(5, 5)]):
        if min(R.pool_out_size(H, k, s, p, ceil), R.pool_out_size(W, k, s, p, ceil)) <= 0:
            continue
        B = R.MAXPOOL_BATCHES[(mi + k + s) % 3]
        Cc = MAX_C[bf16][(mi + p + ceil) % 3]
        rng = np.random.default_rng(1000 * k + 100 * s + 10 * p + ceil + 7 * mi)
        x = R.mixed_sign(rng, (B, Cc, H, W))
        y, raw, kid = graph_op(x, 1, k, k, s, s, p, p, bf16=bf16, ceil=ceil, pad_fill=1024.0)   # every real value is below 2^6
        assert kid == (MAX_BF16 if bf16 else MAX_F32)
        ref = R.maxpool64(R.bf16_round(x) if bf16 else x, k, s, p, ceil)
        assert y.shape == ref.shape
        np.testing.assert_array_equal(y.astype(np.float64), ref)
        check_sentinel(raw, bf16, 0, Cc, B * y.shape[2] * y.shape[3])
        n += 1
    assert n >= 3


def test_maxpool_minus_one_rule():
    x = R.mixed_sign(np.random.default_rng(5), (3, 8, 5, 5))
    y, _, kid = graph_op(x, 1, 2, 2, 2, 2, 1, 1, ceil=1, pad_fill=1024.0)
    assert y.shape[2:] == (3, 3) and kid == MAX_F32
    np.testing.assert_array_equal(y.astype(np.float64), R.maxpool64(x, 2, 2, 1, 1))


@pytest.mark.parametrize("bf16", [0, 1], ids=["f32", "bf16"])
def test_maxpool_channel_range_and_offset(bf16):
    rng = np.random.default_rng(11 + bf16)
    x = R.mixed_sign(rng, (3, 32, 5, 7))
    xr = R.bf16_round(x) if bf16 else x
    off = 16 if bf16 else 8   # (bf16 tensors are addressed in pairs of channel blocks)
    # channels [off, off + 16) of the 32-channel source; the other channels hold larger values, so a wrong plane offset shows
    x2 = x.copy(); x2[:, :off] += 100.0; x2[:, off + 16:] += 100.0
    y, raw, kid = graph_op(x2, 1, 3, 3, 2, 2, 1, 1, bf16=bf16, ceil=1, cin=16, src_c_off=off, pad_fill=1024.0)
    assert kid == (MAX_BF16 if bf16 else MAX_F32)
    np.testing.assert_array_equal(y.astype(np.float64), R.maxpool64(xr[:, off:off + 16], 3, 2, 1, 1))
    check_sentinel(raw, bf16, 0, 16, 3 * y.shape[2] * y.shape[3])
    # written at channel offset 32 of a 96-channel tensor
    Cc = 32
    y, raw, kid = graph_op(x[:, :Cc], 1, 3, 3, 2, 2, 0, 0, bf16=bf16, out_c=96, c_off=32, pad_fill=1024.0)
    np.testing.assert_array_equal(y.astype(np.float64), R.maxpool64(xr[:, :Cc], 3, 2, 0, 0))
    check_sentinel(raw, bf16, 32, Cc, 3 * y.shape[2] * y.shape[3])


@pytest.mark.parametrize("bf16", [0, 1], ids=["f32", "bf16"])
def test_maxpool_edge_values(bf16):
    rng = np.random.default_rng(21)
    x = R.mixed_sign(rng, (3, 16, 13, 13))
    special = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0], np.float32)
    m = rng.uniform(size=x.shape) < 0.35
    x[m] = rng.choice(special, int(m.sum()))
    x[0, :, :4, :4] = np.nan          # windows holding only NaN
    x[1, :, 5:9, 5:9] = -np.inf
    x[2, 0] = np.nan                  # a whole map of NaN
    x[2, 1] = np.where(rng.uniform(size=(13, 13)) < 0.5, 0.0, -0.0)
    for (k, s, p, ceil) in [(3, 2, 1, 1), (2, 2, 0, 1), (3, 1, 1, 0)]:
        y, _, _ = graph_op(x, 1, k, k, s, s, p, p, bf16=bf16, ceil=ceil, pad_fill=1024.0)
        ref = R.maxpool64(R.bf16_round(x) if bf16 else x, k, s, p, ceil)
        assert not np.isnan(ref).any() and (ref == -np.inf).any() and (ref == np.inf).any()
        np.testing.assert_array_equal(R.value_class(y), R.value_class(ref))
        np.testing.assert_array_equal(y.astype(np.float64), ref)


# ---------------------------------------------------------------------------------------------------------------------------------------
# average pool
# ---------------------------------------------------------------------------------------------------------------------------------------
# (geometry, H, W, B list): fp32 and the plain bf16 kernel take every case; the small-map kernel takes the stride-1 same-size cases with H*W <= 256
AVG_CASES = [
    ((3, 3, 1, 1, 1, 1), 1, 1, [3]), ((3, 3, 1, 1, 1, 1), 2, 2, [5]), ((3, 3, 1, 1, 1, 1), 8, 8, [1, 4, 5, 37]), ((3, 3, 1, 1, 1, 1), 5, 7, [8, 15]),
    ((3, 3, 1, 1, 1, 1), 16, 16, [2]), ((3, 3, 1, 1, 1, 1), 17, 16, [2]), ((3, 3, 2, 2, 0, 0), 5, 7, [3]), ((3, 3, 2, 2, 0, 0), 17, 16, [1]),
    ((2, 3, 2, 1, 0, 1), 5, 7, [3]), ((2, 3, 2, 1, 0, 1), 8, 8, [4]), ((2, 3, 2, 1, 0, 1), 2, 2, [37]),
]


def _avg_expected_kernel(mode, geom, H, W):
    kh, kw, sh, sw, ph, pw = geom
    if mode == "f32":
        return AVG_F32
    same = (H + 2 * ph - kh) // sh + 1 == H and (W + 2 * pw - kw) // sw + 1 == W
    return AVG_BF16_SMALL if (sh == 1 and sw == 1 and same and H * W <= 256) else AVG_BF16


@pytest.mark.parametrize("with_bias", [0, 1], ids=["plain", "bias_relu"])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_avgpool(mode, with_bias):
    """Bound, from the kernels' documented order.  With n in-map cells the kernel makes n - 1 inexact fp32 adds (the first, to 0, is exact), rounds
    1 / (kh*kw) once, rounds the product once and, with a bias, rounds one more add: at most n + 2 roundings, each of relative size <= u = 2^-24
    on a quantity of magnitude <= S = sum|x| / (kh*kw) + |bias|.  So |y - y64| <= (n + 2) u S (ReLU is 1-Lipschitz).  bf16: the inputs are
    rounded first (the reference starts from the rounded values) and the fp32 result v is rounded once to bf16's 8 significant bits (unit
    roundoff 2^-8, as fp32's 24 bits give 2^-24): |bf16(v) - v| <= 2^-8 |v| with |v| <= |y64| + (n + 2) u S.  Mixed-sign inputs over 2^-6 .. 2^6: a dropped or extra cell moves y by >= 2^-6 / 9, the bound is < 2^-14."""
    bf16 = mode == "bf16"
    seen = set()
    for ci, (geom, H, W, Bs) in enumerate(AVG_CASES):
        for B in Bs:
            Cc = (16, 24, 48)[(ci + B) % 3] if bf16 else (8, 20, 24)[(ci + B) % 3]
            rng = np.random.default_rng(100 * ci + B)
            x = R.mixed_sign(rng, (B, Cc, H, W))
            bias = R.mixed_sign(rng, (Cc,), -3, 3) if with_bias else None
            y, raw, kid = graph_op(x, 2, *geom, bf16=bf16, pad_fill=1024.0, bias=bias, relu=with_bias)
            assert kid == _avg_expected_kernel(mode, geom, H, W), (geom, H, W, kid)
            seen.add(kid)
            xr = R.bf16_round(x) if bf16 else x
            y64 = R.avgpool64(xr, *geom, bias=bias, relu=bool(with_bias))
            cells = R.avgpool_cells(H, W, *geom)
            S = R.avgpool64(np.abs(xr), *geom) + (np.abs(bias.astype(np.float64))[None, :, None, None] if with_bias else 0.0)
            bound = (cells + 2) * U * S
            if bf16:
                bound = bound + 2.0 ** -8 * (np.abs(y64) + bound)
            err = np.abs(y.astype(np.float64) - y64)
            assert (err <= bound).all(), (geom, H, W, B, float((err / np.maximum(bound, 1e-300)).max()))
            if not with_bias:
                seq = R.avgpool_seq32(xr, *geom)
                np.testing.assert_array_equal(_bits(y), _bits(R.bf16_round(seq) if bf16 else seq))
            check_sentinel(raw, bf16, 0, Cc, B * y.shape[2] * y.shape[3])
    assert seen == ({AVG_BF16, AVG_BF16_SMALL} if bf16 else {AVG_F32})


def test_avgpool_small_kernel_threshold():
    g = (3, 3, 1, 1, 1, 1)
    x = R.mixed_sign(np.random.default_rng(3), (2, 16, 17, 16))
    assert graph_op(x[:, :, :16], 2, *g, bf16=1)[2] == AVG_BF16_SMALL   # H*W = 256: the last shape on the small kernel
    assert graph_op(x, 2, *g, bf16=1)[2] == AVG_BF16                     # 17 x 16: the first on the plain kernel


# ---------------------------------------------------------------------------------------------------------------------------------------
# LRN
# ---------------------------------------------------------------------------------------------------------------------------------------
LRN_SHAPES = {1: (1, 1, 1), 99: (1, 9, 11), 105: (3, 5, 7)}
LRN_FILL_INF = 4e19   # pad pattern 4e19 .. 2e20: finite, and every square is above FLT_MAX (3.4e38)
assert LRN_FILL_INF ** 2 > float(np.finfo(np.float32).max) > 5 * LRN_FILL_INF


def _relerr(y, y64):
    return float((np.abs(y.astype(np.float64) - y64) / np.abs(y64)).max())


def test_lrn(O, capsys):
    ratios = []
    ci = 0
    for Cc in R.LRN_CHANNELS:
        for size in R.LRN_SIZES:
            for pi in ((0, 1) if ci % 5 == 0 else (ci % 2,)):
                alpha, beta, k = R.LRN_PARAMS[pi]
                rows = R.LRN_ROWS[(ci + pi) % 3]
                B, H, W = LRN_SHAPES[rows]
                rng = np.random.default_rng(50 * Cc + size + pi)
                x = R.mixed_sign(rng, (B, Cc, H, W), -3, 7)
                c_off = 16 if (Cc == 13 and size == 5) else 0
                y, raw, kid = graph_op(x, 3, size, size, 1, 1, 0, 0, pad_fill=1e18, lrn=(alpha, beta, k), c_off=c_off)
                assert kid == LRN
                if Cc % 8:   # pad lanes whose squares overflow: the same bits, so no window reads one
                    y2, _, _ = graph_op(x, 3, size, size, 1, 1, 0, 0, pad_fill=LRN_FILL_INF, lrn=(alpha, beta, k), c_off=c_off)
                    np.testing.assert_array_equal(_bits(y2), _bits(y))
                y64 = R.lrn64(x, size, alpha, beta, k)
                e_dev, e_orc = _relerr(y, y64), _relerr(O.lrn(x, size, alpha, beta, k), y64)
                ratios.append((Cc, size, pi, rows, e_dev / U, e_orc / U))
                assert e_dev <= LRN_FACTOR * e_orc, (Cc, size, pi, rows, e_dev / U, e_orc / U)
                check_sentinel(raw, 0, c_off, Cc, rows)
                if Cc % 8:   # the pad lanes of the ragged last block: exactly +0
                    assert (raw[c_off // 8 + Cc // 8, :rows, Cc % 8:] == 0).all()
            ci += 1
    with capsys.disabled():
        print("\nLRN max relative error / 2^-24 (C, size, params, rows, device, oracle):")
        for r in ratios:
            print("  C=%d size=%d p%d rows=%d  device %.2f  oracle %.2f  ratio %.2f" % (r + (r[4] / r[5],)))


def test_lrn_identity_and_pad_lanes():
    for Cc in (5, 13, 24):
        x = R.mixed_sign(np.random.default_rng(Cc), (3, Cc, 5, 7), -3, 7)
        for fill in (1e18, LRN_FILL_INF):
            y, raw, kid = graph_op(x, 3, 5, 5, 1, 1, 0, 0, pad_fill=fill, lrn=(0.0, 0.75, 1.0))
            assert kid == LRN
            np.testing.assert_array_equal(_bits(y), _bits(x))   # alpha = 0, k = 1: x * 1^-beta (a pad lane's inf square would give 0 * inf = NaN)
            if Cc % 8:
                assert (raw[Cc // 8, :105, Cc % 8:] == 0).all()


def test_lrn_edge_values():
    rng = np.random.default_rng(77)
    Cc, size, half = 24, 5, 2
    x = R.mixed_sign(rng, (1, Cc, 9, 11), -3, 7)
    base, _, _ = graph_op(x, 3, size, size, 1, 1, 0, 0, pad_fill=1e18, lrn=R.LRN_PARAMS[0])
    xs = x.copy()
    spots = [(0, 0, 0, np.inf), (23, 8, 10, -np.inf), (7, 4, 4, np.nan), (8, 4, 5, np.inf), (12, 2, 3, np.nan)]
    touched = np.zeros(x.shape, bool)
    for c, yy, xx, v in spots:
        xs[0, c, yy, xx] = v
        touched[0, max(c - half, 0):c + half + 1, yy, xx] = True
    y, _, _ = graph_op(xs, 3, size, size, 1, 1, 0, 0, pad_fill=1e18, lrn=R.LRN_PARAMS[0])
    with np.errstate(all="ignore"):
        y64 = R.lrn64(xs, size, *R.LRN_PARAMS[0])
    np.testing.assert_array_equal(R.value_class(y), R.value_class(y64))
    np.testing.assert_array_equal(_bits(y)[~touched], _bits(base)[~touched])
    assert np.isnan(y[0, 0, 0, 0]) and y[0, 1, 0, 0] == 0 and np.isnan(y[0, 6, 4, 4])


def test_lrn_refusals():
    x = R.mixed_sign(np.random.default_rng(1), (1, 16, 3, 3))
    for kw in (dict(bf16=1, size=5), dict(bf16=0, size=4), dict(bf16=0, size=19)):
        rc, msg = graph_op(x, 3, kw["size"], kw["size"], 1, 1, 0, 0, bf16=kw["bf16"], lrn=R.LRN_PARAMS[0], expect="refusal")
        assert rc == MPN_EINVAL and msg
    y, _, kid = graph_op(x, 3, 5, 5, 1, 1, 0, 0, lrn=R.LRN_PARAMS[0])   # the library is still usable
    assert kid == LRN and np.isfinite(y).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# ROI pooling
# ---------------------------------------------------------------------------------------------------------------------------------------
# name: (bf16, channels, knobs, kernel id)
ROI_KERNELS = {
    "f32_thread": (0, 24, {}, ROI_F32),
    "f32_rows4": (0, 32, {}, ROI_ROWS4),
    "bf16_plain_c48": (1, 48, {}, ROI_BF16),
    "bf16_plain_knob": (1, 32, dict(bf16_fast_pool=2), ROI_BF16),
    "bf16_sorted_c32": (1, 32, {}, ROI_SORTED),
    "bf16_sorted_c64": (1, 64, {}, ROI_SORTED),
}
ROI_N = [1, 5, 37, 130]


@pytest.mark.parametrize("name", list(ROI_KERNELS))
def test_roi_pool(O, name):
    """Every (map, pooled size) case runs BOTH bin rules on the same features and ROI table; N, the scale and roi_stride come from different
    digits of the case index, so each rule meets every N, both scales and both strides.  Tables of 11 or more rows hold every ROI kind of
    R.roi_table (from row 5 on: wholly outside, inverted, one pixel, larger than the image); only the Caffe rule gives empty bins."""
    bf16, Cc, knobs, want = ROI_KERNELS[name]
    i = 0
    seen = {0: set(), 1: set()}
    all_empty_big = 0   # Caffe-rule cases with N >= 11 whose table holds an ROI with every bin empty (-> a map of zeros)
    for (H, W) in R.ROI_MAPS:
        for PH in R.ROI_POOLED:
            N, scale = ROI_N[i % 4], (0.0625, 0.37)[(i // 4) % 2]
            rng = np.random.default_rng(1000 * H + 10 * PH + i)
            feat = R.mixed_sign(rng, (Cc, H, W))
            featr = R.bf16_round(feat) if bf16 else feat
            rois5 = R.roi_table(rng, N, H, W, scale)
            for rule in (0, 1):
                stride = (5, 20)[(i // 8 + rule) % 2]
                pooled, _, _, kids, _ = head_pool(feat, rois_strided(rois5, stride, rng), PH, scale, rule, bf16, pad_fill=1024.0, knobs=knobs)
                assert kids[1] == want and kids[0] == 0 and kids[2] == 0, (name, kids)
                ref = O.roi_pool(featr, rois5, PH, PH, scale, bin_rule=rule)[0]
                np.testing.assert_array_equal(pooled, ref)
                assert _same_bits_up_to_zero_sign(pooled, ref), (name, H, W, PH, N, rule)
                seen[rule].add((N, scale, stride))
                if rule == 0 and N >= 11:
                    rows, cols = R.roi_bins(rois5[5], scale, H, W, PH, PH, 0)
                    if all(b <= a for a, b in rows) or all(b <= a for a, b in cols):
                        assert (ref[5] == 0).all() and (pooled[5] == 0).all() and not np.signbit(pooled[5]).any()
                        all_empty_big += 1
                if rule == 1:
                    assert (ref != 0).all()   # the adaptive rule has no empty bin (mixed-sign features hold no zero)
            i += 1
    assert i == 20
    for rule in (0, 1):
        assert {t[0] for t in seen[rule]} == set(ROI_N) and {t[1] for t in seen[rule]} == {0.0625, 0.37} and {t[2] for t in seen[rule]} == {5, 20}
        assert seen[rule] == {(n, sc, st) for n in ROI_N for sc in (0.0625, 0.37) for st in (5, 20)}, seen[rule]
    assert all_empty_big >= 4, all_empty_big


def _zero_sign_expected(feat, rois5, PH, scale, rule, sorted_kernel):
    """the sign bit of each zero maximum: +0 on the sortable map when the bin holds a +0 (or is empty), the zero met first in the plain kernel"""
    Cc, H, W = feat.shape
    neg = np.zeros((rois5.shape[0], Cc, PH, PH), bool)
    sb = np.signbit(feat)
    for n, r in enumerate(rois5):
        rows, cols = R.roi_bins(r, scale, H, W, PH, PH, rule)
        for a, (y0, y1) in enumerate(rows):
            for b, (x0, x1) in enumerate(cols):
                if y1 <= y0 or x1 <= x0:
                    continue
                blk, sgn = feat[:, y0:y1, x0:x1].reshape(Cc, -1), sb[:, y0:y1, x0:x1].reshape(Cc, -1)
                for c in range(Cc):
                    z = blk[c] == 0
                    if z.any():
                        neg[n, c, a, b] = sgn[c][z].all() if sorted_kernel else sgn[c][np.argmax(z)]
    return neg


def test_roi_pool_bf16_sorted_vs_plain_edge_values():
    """Both bf16 kernels on the same NaN / +-inf / +-0 features.  Values and classes agree (NaNs ignored, only-NaN -> -inf, empty bin -> 0); the
    bits agree except the sign of a zero maximum, which each kernel gives by its own rule (pinned here, stated in include/mpn.h)."""
    rng = np.random.default_rng(404)
    Cc, H, W, PH, scale = 32, 9, 13, 6, 0.25
    feat = -np.abs(R.mixed_sign(rng, (Cc, H, W)))
    m = rng.uniform(size=feat.shape)
    feat[m < 0.45] = rng.choice(np.array([0.0, -0.0], np.float32), int((m < 0.45).sum()))
    feat[(m >= 0.45) & (m < 0.6)] = np.nan
    feat[(m >= 0.6) & (m < 0.63)] = np.inf
    feat[1] = np.nan                                   # bins of NaN alone
    feat[2] = np.where(m[2] < 0.5, np.nan, -np.inf)
    feat[3] = -np.nan                                  # negative NaNs
    feat[4] = np.where(m[4] < 0.3, -0.0, feat[4])
    rois5 = R.roi_table(rng, 30, H, W, scale)
    for rule in (0, 1):
        s_out, _, _, ks, _ = head_pool(feat, rois5, PH, scale, rule, 1, pad_fill=1024.0)
        p_out, _, _, kp, _ = head_pool(feat, rois5, PH, scale, rule, 1, pad_fill=1024.0, knobs=dict(bf16_fast_pool=2))
        assert ks[1] == ROI_SORTED and kp[1] == ROI_BF16
        ref = R.roi_pool64(R.bf16_round(feat), rois5, PH, PH, scale, rule)
        assert not np.isnan(ref).any() and (ref == -np.inf).any() and (ref == np.inf).any() and (ref == 0).any()
        for got, is_sorted in ((s_out, True), (p_out, False)):
            np.testing.assert_array_equal(R.value_class(got), R.value_class(ref))
            np.testing.assert_array_equal(got.astype(np.float64), ref)
            zero = ref == 0
            neg = _zero_sign_expected(feat, rois5, PH, scale, rule, is_sorted)
            np.testing.assert_array_equal(np.signbit(got)[zero], neg[zero])
        assert _same_bits_up_to_zero_sign(s_out, p_out)
        assert (np.signbit(s_out) != np.signbit(p_out))[ref == 0].any()   # the rules do differ on these features


# ---------------------------------------------------------------------------------------------------------------------------------------
# fused ROI max-pool
# ---------------------------------------------------------------------------------------------------------------------------------------
def _height_rois(H, W):
    """windows of every height 1 .. H at scale 1/16: (y - 1) / 16 is an integer, so the rows are exact"""
    rows = []
    for h in range(1, H + 1):
        a = (h * 7) % (H - h + 1)
        rows.append([1.0, 16.0 * (W // 5) + 1, 16.0 * a + 1, 16.0 * (W - 1 - W // 7) + 1, 16.0 * (a + h - 1) + 1])
    return np.array(rows, np.float32)


@pytest.mark.parametrize("tables", [1, 0], ids=["tables", "no_tables"])
@pytest.mark.parametrize("PH,k,s,p", R.ROIMAX_GEOMS)
def test_roi_maxpool_fused(O, PH, k, s, p, tables):
    knobs = {} if tables else dict(graph_fuse=511 & ~64)
    for mi, (H, W) in enumerate(R.ROIMAX_MAPS):
        levels = (H.bit_length() - 1) if (tables and H > 1) else 0
        for negative in (True, False):
            rng = np.random.default_rng(100 * PH + 10 * mi + negative)
            feat = R.mixed_sign(rng, (32, H, W))
            if negative:
                feat = -np.abs(feat)   # an empty bin's 0 must win
            rois5 = np.concatenate([R.roi_table(rng, 22, H, W, 0.0625), _height_rois(H, W)])
            stride = 20 if negative else 5
            pooled, mp, _, kids, lv = head_pool(feat, rois_strided(rois5, stride, rng), PH, 0.0625, 0, 1, op=(k, s, p), pad_fill=1024.0, knobs=knobs)
            assert kids[1] == ROI_SORTED and kids[0] == 0 and lv == levels, (kids, lv)
            assert kids[2] == (ROIMAX_SORTED_TABLES if levels else ROIMAX_SORTED), kids
            ref1 = O.roi_pool(R.bf16_round(feat), rois5, PH, PH, 0.0625, bin_rule=0)[0]
            ref2 = O.maxpool2d_mode(ref1, k, s, p, 0)
            assert _same_bits_up_to_zero_sign(pooled, ref1)
            np.testing.assert_array_equal(mp, ref2)
            assert _same_bits_up_to_zero_sign(mp, ref2), (H, W, negative)
            if negative:
                assert (ref2 == 0).any() and (ref2[5] == 0).all()   # bins outside the map; the ROI wholly outside


def _nan_features(rng, Cc, H, W):
    feat = R.mixed_sign(rng, (Cc, H, W))
    m = rng.uniform(size=feat.shape)
    feat[m < 0.3] = np.nan
    feat[(m >= 0.3) & (m < 0.34)] = np.inf
    feat[(m >= 0.34) & (m < 0.4)] = -np.inf
    feat[1] = np.nan                                   # windows of NaN alone
    feat[2] = -np.nan
    feat[3] = np.where(m[3] < 0.5, np.nan, -np.inf)
    feat[4] = np.where(m[4] < 0.5, np.nan, feat[4])
    feat[5, :, ::2] = np.nan                           # NaN in every window column (the range-max tables read rows apart)
    feat[6, ::2] = np.nan
    return feat


@pytest.mark.parametrize("tables", [1, 0], ids=["tables", "no_tables"])
def test_roi_maxpool_fused_ignores_nan(tables):
    """NaN / +-inf features through the fused kernel (and, with tables, vmax_level_sorted_kernel's range-max levels): NaNs are ignored, a window
    of NaNs alone gives -inf, an empty bin's 0 joins the max — the float64 two-step sequence, as values and classes (include/mpn.h)."""
    knobs = {} if tables else dict(graph_fuse=511 & ~64)
    rng = np.random.default_rng(909)
    H, W, scale = 13, 9, 0.0625
    feat = _nan_features(rng, 32, H, W)
    rois5 = np.concatenate([R.roi_table(rng, 22, H, W, scale), _height_rois(H, W)])
    for (PH, k, s, p) in R.ROIMAX_GEOMS:
        pooled, mp, _, kids, lv = head_pool(feat, rois5, PH, scale, 0, 1, op=(k, s, p), pad_fill=1024.0, knobs=knobs)
        assert kids[1] == ROI_SORTED and kids[0] == 0 and lv == (3 if tables else 0), (kids, lv)
        assert kids[2] == (ROIMAX_SORTED_TABLES if tables else ROIMAX_SORTED), kids
        featr = R.bf16_round(feat)
        ref1 = R.roi_pool64(featr, rois5, PH, PH, scale, 0)
        ref2 = R.maxpool64(ref1, k, s, p, 0)
        for got, ref in ((pooled, ref1), (mp, ref2)):
            assert not np.isnan(ref).any() and (ref == -np.inf).any() and (ref == np.inf).any() and (ref == 0).any()
            np.testing.assert_array_equal(R.value_class(got), R.value_class(ref))
            np.testing.assert_array_equal(got.astype(np.float64), ref)


@pytest.mark.parametrize("name", ["f32_thread", "f32_rows4", "bf16_plain_c48"])
def test_roi_pool_ignores_nan(name):
    """the kernels that compare floats (f > m from -inf): the same rule, both bin rules"""
    bf16, Cc, knobs, want = ROI_KERNELS[name]
    rng = np.random.default_rng(910)
    H, W, scale, PH = 13, 9, 0.0625, 6
    feat = _nan_features(rng, Cc, H, W)
    rois5 = R.roi_table(rng, 22, H, W, scale)
    for rule in (0, 1):
        pooled, _, _, kids, _ = head_pool(feat, rois5, PH, scale, rule, bf16, pad_fill=1024.0, knobs=knobs)
        assert kids[1] == want
        ref = R.roi_pool64(R.bf16_round(feat) if bf16 else feat, rois5, PH, PH, scale, rule)
        assert not np.isnan(ref).any() and (ref == -np.inf).any() and (ref == np.inf).any()
        np.testing.assert_array_equal(R.value_class(pooled), R.value_class(ref))
        np.testing.assert_array_equal(pooled.astype(np.float64), ref)


def test_roi_maxpool_adaptive_rule_runs_as_an_ordinary_pool(O):
    rng = np.random.default_rng(8)
    feat = R.mixed_sign(rng, (32, 9, 13))
    rois5 = R.roi_table(rng, 15, 9, 13, 0.25)
    pooled, mp, _, kids, lv = head_pool(feat, rois5, 7, 0.25, 1, 1, op=(3, 2, 1), pad_fill=1024.0)
    assert kids[1] == ROI_SORTED and kids[2] == 0 and kids[0] == MAX_BF16 and lv == 0, kids
    ref1 = O.roi_pool(R.bf16_round(feat), rois5, 7, 7, 0.25, bin_rule=1)[0]
    assert _same_bits_up_to_zero_sign(pooled, ref1)
    assert _same_bits_up_to_zero_sign(mp, O.maxpool2d_mode(ref1, 3, 2, 1, 0))
    # fp32: always the two-step sequence
    pooled, mp, _, kids, _ = head_pool(feat, rois5, 7, 0.25, 0, 0, op=(3, 2, 1), pad_fill=1024.0)
    assert kids[1] == ROI_ROWS4 and kids[2] == 0 and kids[0] == MAX_F32, kids
    assert _same_bits_up_to_zero_sign(mp, O.maxpool2d_mode(O.roi_pool(feat, rois5, 7, 7, 0.25, bin_rule=0)[0], 3, 2, 1, 0))


# ---------------------------------------------------------------------------------------------------------------------------------------
# closing average
# ---------------------------------------------------------------------------------------------------------------------------------------
GAVG_KERNELS = {"f32": (0, 24, {}, GAVG_F32), "bf16_plain": (1, 32, dict(bf16_fast_pool=1), GAVG_BF16), "bf16_lds": (1, 48, {}, GAVG_BF16_LDS)}


@pytest.mark.parametrize("name", list(GAVG_KERNELS))
def test_closing_average(name):
    """Bound as in test_avgpool with n = H*W cells and no bias: n - 1 adds, the rounding of 1 / n and of the product: (n + 1) u mean|x| <=
    (n + 2) u mean|x|.  The output is fp32 for both dtypes, so there is no further rounding."""
    bf16, Cc, knobs, want = GAVG_KERNELS[name]
    i = 0
    for PH in (1, 6, 7, 8):
        assert PH * PH in R.GAVG_HW
        for N in R.GAVG_N:
            rng = np.random.default_rng(10 * PH + N)
            H, W = 12, 17
            feat = R.mixed_sign(rng, (Cc, H, W))
            rois5 = R.roi_table(rng, N, H, W, 0.25)
            Mp = N + 1 + i % 3
            pooled, _, c8, kids, _ = head_pool(feat, rois5, PH, 0.25, i % 2, bf16, pad_fill=1024.0, Mp=Mp, knobs=knobs)
            assert kids[3] == want, (name, kids)
            got = c8.view(np.float32)                                # [Cb, Mp, 8]
            rows = got[:, :N].transpose(1, 0, 2).reshape(N, -1)[:, :Cc]   # [N, C]
            np.testing.assert_array_equal(_bits(rows), _bits(R.global_avg_seq32(pooled)))
            y64 = R.global_avg64(pooled)
            bound = (PH * PH + 2) * U * np.abs(pooled).astype(np.float64).mean(axis=(2, 3))
            assert (np.abs(rows.astype(np.float64) - y64) <= bound).all()
            assert (c8[:, N:] == SENT32).all(), "rows >= N were written"
            i += 1


# ---------------------------------------------------------------------------------------------------------------------------------------
# repeatability
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_repeatable():
    rng = np.random.default_rng(2)
    x = R.mixed_sign(rng, (5, 24, 8, 8))
    for bf16 in (0, 1):
        for args in ((1, 3, 3, 2, 2, 1, 1), (2, 3, 3, 1, 1, 1, 1)):
            a, b = graph_op(x, *args, bf16=bf16), graph_op(x, *args, bf16=bf16)
            assert np.array_equal(a[1], b[1]) and a[2] == b[2]
    a, b = (graph_op(x, 3, 5, 5, 1, 1, 0, 0, lrn=R.LRN_PARAMS[0], pad_fill=1e18) for _ in range(2))
    assert np.array_equal(a[1], b[1])
    feat = R.mixed_sign(rng, (32, 9, 13))
    rois5 = R.roi_table(rng, 37, 9, 13, 0.25)
    for bf16 in (0, 1):
        a, b = (head_pool(feat, rois5, 7, 0.25, 0, bf16, op=(3, 2, 1)) for _ in range(2))
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(a[2], b[2]) and a[3] == b[3]
