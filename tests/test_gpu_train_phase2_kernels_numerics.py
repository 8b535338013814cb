"""The kernels between MultiPathNet's mix layers and its conv block (mpn_mpnet_train_begin_conv), one launch at a
time, against float64 and against NumPy restatements of the orders train.h documents: normalize_backward_kernel,
roi_pool_backward_add_kernel, int_to_float_kernel, and linear_dgrad_c8 in the form the tower backward launches — K = c5 on a packed weight
wider than K, one launch over (PP - 1) * Mp + B rows with stale rows between the segments.  Until now they were reached only through whole
training steps on two networks with c5 = 48 or 40 and PP = 49.

The kernels are called through the mpn_debug_* pass-throughs of train_debug.hip (debug flavour only).  Layouts, orders, references and
input sets are tests/train_phase2_kernels_np.py's and tests/train_phase2_np.py's, checked on the CPU in
tests/test_train_phase2_kernels_ref_cpu.py.  Buf, twice, the ACC lines and the sentinel helpers are the two existing kernel modules'.
DESIGN.md section 13.16.

Common setup: every device buffer sits between two guard zones of 256 sentinel NaNs (0x7FA5A5A5).  What the contract says is not written
holds the sentinel and must keep its bits: rows >= B and the pad lanes of dx; the halo, the pitch padding and the pad lanes of the gather's
C8P map; dx chunks >= K / 8 and rows beyond the launch's of the prefix launch; the float behind n.  What it says is not read holds NaN: rows
>= B and the pad lanes of x, y and g; the rows outside [n0, n1) of the gather's g and rois (their argmax points at cell 0), the batch column
and, at roi_stride 20 and 7, the floats of a table row outside the selected five; rows n >= N of a packed weight.  Every case runs twice
on fresh buffers: the same bits.  Every comparison prints an ACC line.  Inputs are read back unchanged.

Tiers.
  bit-exact   normalize_backward on operands of at most 12, and of at most 16, significant bits (every fused multiply-add of the emulation
              is then exact in float64, shown on the CPU) equals normalize_backward_f32 — 256 strided fma chains, the tree 128 .. 1, then the elementwise
              tail; an all-zero row gives s = mul / sqrt(1e-10f) and dx = s g, a row with g = 0 gives the restatement's zeros.  The gather
              from a map that holds values equals the chain restatement (one call and three in a row), cells nothing is added to keep
              their bits (-0.0, a NaN's payload), on a zeroed map it equals mpn_debug_roi_pool_backward, windows = 1 equals windows = 0,
              n0 = n1 leaves every bit.  int_to_float equals np.float32(int).
  exact       integer operands in [-2, 2]: both Normalize sums are integers below 2^24, so dx equals the tail evaluated from the float64
              sums whatever the order — a dropped or doubled entry shows with no tolerance.  The prefix launch of linear_dgrad_c8 equals
              float64, the same launch with the stale rows zeroed and a launch on a weight packed for K alone, bit for bit.
  derived     full-mantissa operands: |dx - normalize_backward64| <= normalize_backward_bound (L = ceil(ceil(C / 8) * PP * 8 / 256));
              the gather with a synthetic argmax (many rows and bins into three cells) within (terms + 1) * 2^-23 * (|start| + sum |g|).

c5 % 8 != 0.  A handle refuses a trunk whose last layer is no multiple of 8 channels wide (create: feat_c % 8 == 0;
tests/test_gpu_train_phase2.py asserts the refusal), so the driver never launches these kernels with a pad lane: the C % 8 != 0 cases
here document the kernels' own contract — which alloc_tower_train_state's (c5 + 7) / 8 sizing matches — not a path of the product.  For
the same reason the driver never launches linear_dgrad_c8 with K = 44.  What the kernel does there is tested as it is: on a weight
packed for K = 44 alone the four pad lanes of chunk 5 come out +-0 (the pack's pad lanes are +0.0); on the mix weight's real packing
(Kfull columns, contiguous) lanes 44 .. 47 of chunk 5 would hold the NEXT slab's first four columns and receive their products —
the slabs are not padded to 8, which is why the handle's refusal is needed.

What the module found.  No kernel computes a wrong value or touches what its contract says it does not.  About the tests: a product of
two 12-bit operands is an fp32 value, so the 12-bit set that makes the fma emulation exact cannot tell an fma from a multiply and an add;
the 16-bit set (magnitudes in [2^-2, 2^2): products of 32 bits, product + partial still exact in float64) can, where a thread owns several
entries.

MEASURED on the MI355X (largest observed error / bound per family, from the ACC lines; DESIGN.md section 13.16 has the same table):
  normalize_backward_c8, derived set   0.252 (C 40, PP 49, B 70), 0.039 at L = 98; 9 comparisons        (CPU, stated order in fp32: 0.252 / 0.039)
  gather on a synthetic arg-max        0.161 (7 x 7, C 12), 3 cases; bit-equal to the fp32 chain         (CPU, the sequential chain: 0.161)
  339 bit-exact comparisons, none differing; two runs in a row print the same 363 ACC lines.  The module's wall time is 4.3 s (41 tests).

Mutations tried on scratch copies of the debug library (MI355X; each only drops work or changes arithmetic, every access in bounds), with
the tests that fail on each:
  normalize_backward_kernel: the tree from 64 / a stride of 128 in the first pass   test_normalize_backward, the six shapes with E >= 256
    x*x + ss and y*g + d without the fma                                            test_normalize_backward, the four shapes with E >= 784 (16-bit set)
    the pad-lane test > for >=                                                      test_normalize_backward, the five shapes with C % 8 != 0
    coef with mul for mul^2                                                         test_normalize_backward (all 9)
    the second pass dropping the last entry                                         test_normalize_backward, the four shapes with C % 8 == 0
  roi_pool_backward_add_kernel: the chain from 0 instead of *o / rows descending /
    the arg-max compared with cell + 1                                              test_roi_pool_backward_add (all 14), ..._synthetic_argmax (all 3)
    bins descending                                                                 test_roi_pool_backward_add (12: not the one-bin pooling), ..._synthetic_argmax
    roi_stride ignored (5)                                                          test_roi_pool_backward_add (13: not the 1 x 1 map under rule 1)
    1u << (pw & 15)                                                                 test_roi_pool_backward_add, the four 32 x 32 cases
  int_to_float_kernel's tail one short                                              test_int_to_float (all 5)
  linear_dgrad_c8: nchunks from the weight's K (rounded to 64) / every row reading
    row 0 of g                                                                      test_linear_dgrad_prefix_launch (all 8)
    only the m_ok guard of the g load dropped (rows >= B read row 0)                 none: an equivalent mutant, those rows' results are never stored
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_train_conv_kernels_numerics as TCK  # noqa: E402  (_acc with its per-family maximum, _bits_acc, _is_sent, _sent_i)
import test_gpu_train_kernels_numerics as T  # noqa: E402  (Buf, twice and the sentinel helpers: one setup for the three modules)
import train_conv_kernels_np as K  # noqa: E402
import train_kernels_np as R  # noqa: E402
import train_phase2_kernels_np as Q  # noqa: E402
import train_phase2_np as P2  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENT_F = R.SENT_F
MPN_EINVAL = -1
Buf, twice, NULL = T.Buf, T.twice, T.NULL
_sent, _same = T._sent, T._same
_acc, _bits_acc, _is_sent, _sent_i = TCK._acc, TCK._bits_acc, TCK._is_sent, TCK._sent_i
cf, ci, cs, vp = C.c_float, C.c_int, C.c_size_t, C.c_void_p
NAN = F32(np.nan)


@functools.lru_cache(maxsize=None)
def _dbg():
    lib = TCK._dbg()
    b = [vp, cs]
    lib.mpn_debug_normalize_backward_c8.argtypes = b + b + b + b + [ci, ci, ci, ci, cf]
    lib.mpn_debug_roi_pool_backward_add.argtypes = b + b + b + [ci] * 11 + [cf, ci] + b
    lib.mpn_debug_int_to_float.argtypes = b + [cs] + b
    return lib


def _err():
    return _dbg().mpn_last_error().decode()


def _ok(rc):
    assert rc == 0, (rc, _err())


def _invalid(rc):
    assert rc == MPN_EINVAL and "invalid argument" in _err(), (rc, _err())


def _short(rc, name):
    assert rc == MPN_EINVAL and "footprint" in _err() and (name + " holds") in _err(), (rc, name, _err())


# ---- normalize_backward_c8 -------------------------------------------------------------------------------------------------------------
def _run_norm(x, y, g, case, mul):
    """x, y, g [B, C, PP] -> dx [B, C, PP], after checking everything the launch must leave alone"""
    C_, PP, B, Mp = case
    xs, ys, gs = (Q.slab_pack(a, Mp, fill=NAN) for a in (x, y, g))   # rows >= B and the pad lanes of the last block: never read
    real = Q.slab_real(B, C_, PP, Mp)

    def call():
        xb, yb, gb, db = Buf(xs), Buf(ys), Buf(gs), Buf(_sent(*xs.shape))
        _ok(_dbg().mpn_debug_normalize_backward_c8(*xb.a, *yb.a, *gb.a, *db.a, Mp, B, C_, PP, mul))
        d = db.read()
        assert _same(xb.read(), xs) and _same(yb.read(), ys) and _same(gb.read(), gs), "an input was written"
        return (d,)
    d = twice(call)[0]
    assert _is_sent(d[~real]), "a row >= B or a pad lane of dx was written"
    return Q.slab_unpack(d, B, C_, PP)


@pytest.mark.parametrize("case", Q.NORM_CASES, ids=["C%d_PP%d_B%d_Mp%d" % c for c in Q.NORM_CASES])
def test_normalize_backward(dev, case):
    C_, PP, B, Mp = case
    mul = Q.norm_mul(case)
    tag = "C%d PP%d B%d Mp%d mul %g" % (case + (mul,))
    # bit-exact: the stated order, on the 12-bit set and on the 16-bit set (whose products a plain multiply would round)
    for tier in Q.BIT_TIERS:
        x, y, g = Q.norm_inputs(case, tier)
        got = _run_norm(x, y, g, case, mul)
        ref = P2.normalize_backward_f32(x, y, g, mul)
        assert np.isfinite(got).all()
        _bits_acc("normalize_backward stated order, %s %s" % (tier, tag), got, ref)
        if B >= 2:   # the all-zero row: s = mul / sqrt(1e-10f), dx = s g
            s = F32(F32(mul) / np.sqrt(F32(1e-10)))
            _bits_acc("normalize_backward zero row, %s %s" % (tier, tag), got[B - 1], (s * g[B - 1]).astype(F32))
        if B >= 3:   # g = 0: +-0 with the restatement's bits (asserted above), nothing else
            assert not got[0].any()
    # exact: integer operands, the tail evaluated from the float64 sums
    x, y, g = Q.norm_inputs(case, "exact")
    _bits_acc("normalize_backward exact " + tag, _run_norm(x, y, g, case, mul), Q.normalize_backward_exact(x, y, g, mul))
    # derived: full-mantissa operands against float64
    x, y, g = Q.norm_inputs(case, "derived")
    got = _run_norm(x, y, g, case, mul)
    _acc("normalize_backward", tag, np.abs(got.astype(F64) - P2.normalize_backward64(x, y, g, mul)), P2.normalize_backward_bound(x, y, g, mul))


def test_normalize_backward_refusals(dev):
    C_, PP, B, Mp = 9, 7, 4, 5
    n = Q.cdiv(C_, 8) * PP * Mp * 8
    xb, yb, gb, db = (Buf(_sent(n)) for _ in range(4))

    def call(x_=xb.a, y_=yb.a, g_=gb.a, d_=db.a, Mp_=Mp, B_=B, C2=C_, PP_=PP, mul=1000.0):
        return _dbg().mpn_debug_normalize_backward_c8(*x_, *y_, *g_, *d_, Mp_, B_, C2, PP_, mul)
    for kw in (dict(B_=0), dict(Mp_=B - 1), dict(C2=0), dict(PP_=0), dict(mul=0.0), dict(mul=-1.0), dict(B_=-1)):
        _invalid(call(**kw))
    for kw, name in ((dict(x_=xb.short()), "d_x_c8"), (dict(y_=yb.short()), "d_y_c8"), (dict(g_=gb.short()), "d_g_c8"), (dict(d_=db.short()), "d_dx_c8")):
        _short(call(**kw), name)
    # a larger C at the same buffers: the footprint grows by one channel block
    _short(call(C2=17), "d_x_c8")
    for b in (xb, yb, gb, db):
        assert _is_sent(b.read()), "a refused call wrote something"


# ---- roi_pool_backward_add -------------------------------------------------------------------------------------------------------------
ROI_MP = 128


def _forward_argmax(feat, rois, case, rule, stride, region):
    """the product's forward (roi_pool_c8, form 0) at the same scale, bin rule and roi_stride -> arg-max [N, C, PP] int32"""
    C_, H, W, PH, PW, N = case
    PP = PH * PW
    table = Q.roi_table(rois, stride, region)   # the floats of a table row outside the selected five: NaN
    fb, rb = Buf(K.c8p_pack(feat, pad=0.0, halo=F32(2.0 ** 100), pitch=F32(2.0 ** 100))), Buf(table)
    xb, ab = Buf(_sent(K.cdiv(C_, 8) * PP * ROI_MP * 8)), Buf(_sent_i(N * C_ * PP))
    _ok(_dbg().mpn_debug_roi_pool_form(0, *fb.a, C_, H, W, 0, 0, vp(rb.ptr + 20 * region), rb.n - 5 * region, stride, N, PH, PW, K.ROI_SCALE, rule, ROI_MP,
                                       0, 1.0, *xb.a, *ab.a, *NULL))
    return ab.read().reshape(N, C_, PP)


def _run_add(map0, g, am, rois, case, rule, n0, n1, windows, stride=5, region=0):
    """one call on the C8P map built from map0 [C, H, W] -> the map's interior [C, H, W], after checking what the launch must leave alone"""
    C_, H, W, PH, PW, N = case
    gq, aq, rq = g.copy(), am.copy(), rois.copy()
    out_rows = np.ones(N, bool)
    out_rows[n0:n1] = False
    gq[out_rows], aq[out_rows], rq[out_rows] = np.nan, 0, np.nan   # rows outside [n0, n1): never read
    rq[:, 0] = np.nan                                               # the batch column: never read (by_batch = 0)
    gin = K.roi_g_c8(gq, ROI_MP, fill=SENT_F)                       # lanes c >= C and rows >= N: never read
    table = Q.roi_table(rq, stride, region)                         # the floats of a table row outside the selected five: NaN
    m0 = K.c8p_pack(map0, pad=SENT_F, halo=SENT_F, pitch=SENT_F)
    real, pad, outside = K.c8p_masks(C_, H, W)

    def call():
        gb, ab, rb, ob = Buf(gin), Buf(aq), Buf(table), Buf(m0)
        _ok(_dbg().mpn_debug_roi_pool_backward_add(*gb.a, *ab.a, vp(rb.ptr + 20 * region), rb.n - 5 * region, N, stride, ROI_MP, n0, n1, C_, H, W, PH, PW,
                                                   windows, K.ROI_SCALE, rule, *ob.a))
        o = ob.read()
        assert _same(gb.read(), gin) and _same(ab.read(), aq) and _same(rb.read(), table), "an input was written"
        return (o,)
    o = twice(call)[0]
    assert _is_sent(o[pad]) and _is_sent(o[outside]), "a pad lane, the halo or the pitch padding of the map was written"
    return K.c8p_unpack(o, C_, H, W)


def _plain_backward(g, am, rois, case, rule):
    """mpn_debug_roi_pool_backward, layout 1, all rows, windows 0, roi_stride 5 -> [C, H, W]"""
    C_, H, W, PH, PW, N = case
    gb, ab, rb = Buf(K.roi_g_c8(g, ROI_MP, fill=SENT_F)), Buf(am), Buf(rois)
    ob = Buf(_sent(*K.c8p_masks(C_, H, W)[0].shape))
    _ok(_dbg().mpn_debug_roi_pool_backward(*gb.a, *ab.a, *rb.a, N, 1, ROI_MP, 0, 0, N, 1, C_, H, W, PH, PW, 0, K.ROI_SCALE, rule, *ob.a))
    return K.c8p_unpack(ob.read(), C_, H, W)


@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("case", Q.GATHER_CASES, ids=["C%d_%dx%d_p%dx%d_N%d" % c for c in Q.GATHER_CASES])
def test_roi_pool_backward_add(dev, case, rule):
    C_, H, W, PH, PW, N = case
    feat, rois, g, own = Q.gather_inputs(case, rule)
    tag = "C%d %dx%d p%dx%d N%d rule %d" % (case + (rule,))
    zero = np.zeros((C_, H, W), F32)
    plain = _plain_backward(g, own, rois, case, rule)
    am2 = K.window_argmax(feat, rois, PH, PW, K.ROI_SCALE, 1 - rule)
    am3 = Q.third_argmax(own)
    m0, special = Q.start_map(case, [own, am2, am3])
    for stride, region in Q.ROI_STRIDES:
        st = "%s stride %d region %d" % (tag, stride, region)
        am = _forward_argmax(feat, rois, case, rule, stride, region)
        assert np.array_equal(am, own), "the forward's arg-max differs from roi_bin_bounds' windows restated in NumPy"
        # (a) on a zeroed map: roi_pool_backward's result; (d) windows = 1 equals windows = 0
        z0 = _run_add(zero, g, am, rois, case, rule, 0, N, 0, stride, region)
        _bits_acc("gather on a zeroed map == roi_pool_backward " + st, z0, plain)
        _bits_acc("gather windows 1 == 0, zeroed map " + st, _run_add(zero, g, am, rois, case, rule, 0, N, 1, stride, region), z0)
        # (b) on a map that holds values: the chain continues from them; (e) the rows outside [n0, n1) are not read; (f) n0 = n1
        ranges = K.roi_row_ranges(N) if (stride, region) in ((5, 0), (20, 3)) else [(0, N)]
        for n0, n1 in ranges:
            ref = Q.gather_chain(m0, g, am, n0, n1, W)
            got = _run_add(m0, g, am, rois, case, rule, n0, n1, 1, stride, region)
            _bits_acc("gather chain from a map %s rows [%d, %d) windows 1" % (st, n0, n1), got, ref, nanpos=True)
            assert _same(got, ref), "a cell's bits differ (the NaN's payload or -0.0 among them)"
            if n0 == n1:
                assert _same(got, m0), "n0 = n1 changed the map"
            if stride == 5:
                got0 = _run_add(m0, g, am, rois, case, rule, n0, n1, 0, stride, region)
                assert _same(got0, got), "windows = 0 differs from windows = 1"
    for c0, i0 in special:
        assert R.bits(got.reshape(C_, -1)[c0, i0]) == R.bits(m0.reshape(C_, -1)[c0, i0])
    # (c) three calls in a row with different g and argmax: the chain over towers (windows 0: the second and third argmax are not this
    # rule's forward's)
    rng = np.random.default_rng(list(case) + [rule, 59])
    gs = [g, R.draw(rng, g.shape), R.draw(rng, g.shape)]
    cur, ref = m0, m0
    for t, (gt, amt) in enumerate(zip(gs, (own, am2, am3))):
        cur = _run_add(cur, gt, amt, rois, case, rule, 0, N, 0, 20, 1)
        ref = Q.gather_chain(ref, gt, amt, 0, N, W)
        assert _same(cur, ref), "call %d of the chain" % t
    _bits_acc("gather three calls in a row " + tag, cur, ref, nanpos=True)


@pytest.mark.parametrize("PH,PW,C_,B", K.ROI_SYNTH_CASES)
def test_roi_pool_backward_add_synthetic_argmax(dev, PH, PW, C_, B):
    """arg-max values no forward produced (any cell, many rows and bins into three cells, -1), windows = 0, from a map of random values:
    the chain's bits and the derived bound against float64.  More than 32 bins along a side: windows = 1 is refused, windows = 0 right."""
    H, W, N = K.ROI_SYNTH_MAP
    case = (C_, H, W, PH, PW, N)
    am, g, rois = K.roi_synth_inputs(PH, PW, C_, B)
    m0 = R.draw(np.random.default_rng([PH, PW, C_, 53]), (C_, H, W))
    got = _run_add(m0, g, am, rois, case, 0, 0, N, 0, 7, 0)
    _bits_acc("gather synthetic arg-max p%dx%d C%d" % (PH, PW, C_), got, Q.gather_chain(m0, g, am, 0, N, W))
    _acc("roi_pool_backward_add chain", "p%dx%d C%d" % (PH, PW, C_), np.abs(got.astype(F64) - Q.gather_chain(m0, g, am, 0, N, W, dtype=F64)),
         Q.gather_bound(m0, g, am, 0, N, W))
    if max(PH, PW) > 32:
        gb, ab, rb, ob = Buf(K.roi_g_c8(g, ROI_MP, fill=SENT_F)), Buf(am), Buf(rois), Buf(_sent(*K.c8p_masks(C_, H, W)[0].shape))
        _invalid(_dbg().mpn_debug_roi_pool_backward_add(*gb.a, *ab.a, *rb.a, N, 5, ROI_MP, 0, N, C_, H, W, PH, PW, 1, K.ROI_SCALE, 0, *ob.a))
        assert _is_sent(ob.read())


def test_roi_pool_backward_add_refusals(dev):
    N, C_, H, W, PH, PW = 5, 12, 5, 7, 3, 5
    PP = PH * PW
    gb, ab, rb = Buf(_sent(2 * PP * ROI_MP * 8)), Buf(_sent_i(N * C_ * PP)), Buf(_sent(N * 5))
    r20, ob = Buf(_sent((N - 1) * 20 + 5)), Buf(_sent(int(np.prod(K.c8p_masks(C_, H, W)[0].shape))))

    def call(g_=gb.a, a_=ab.a, r_=rb.a, o_=ob.a, stride=5, Mp_=ROI_MP, n0=0, n1=N, rule=0, PH_=PH, PW_=PW, windows=0, C2=C_):
        return _dbg().mpn_debug_roi_pool_backward_add(*g_, *a_, *r_, N, stride, Mp_, n0, n1, C2, H, W, PH_, PW_, windows, 0.25, rule, *o_)
    for kw in (dict(stride=4), dict(stride=0), dict(n1=N + 1), dict(n0=3, n1=2), dict(n0=-1), dict(Mp_=N - 1), dict(rule=2), dict(PH_=0), dict(C2=0)):
        _invalid(call(**kw))
    for kw, name in ((dict(g_=gb.short()), "d_g"), (dict(a_=ab.short()), "d_argmax"), (dict(r_=rb.short()), "d_rois"), (dict(o_=ob.short()), "d_out"),
                     (dict(r_=rb.a, stride=20), "d_rois"), (dict(r_=r20.short(), stride=20), "d_rois"), (dict(C2=17), "d_argmax")):
        _short(call(**kw), name)
    for b in (gb, ab, rb, r20, ob):
        assert _is_sent(b.read()), "a refused call wrote something"


# ---- int_to_float ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", Q.I2F_N)
def test_int_to_float(dev, n):
    for k, v in enumerate(Q.i2f_inputs(n)):
        def call():
            ib, ob = Buf(v), Buf(_sent(n + 19))
            _ok(_dbg().mpn_debug_int_to_float(*ib.a, n, *ob.a))
            assert np.array_equal(ib.read(), v)
            return (ob.read(),)
        got = twice(call)[0]
        _bits_acc("int_to_float n %d set %d" % (n, k), got[:n], v.astype(F32))
        assert _is_sent(got[n:]), "a float behind n was written"
    ib, ob = Buf(v), Buf(_sent(n + 19))
    _short(_dbg().mpn_debug_int_to_float(*ib.short(), n, *ob.a), "d_in")
    _short(_dbg().mpn_debug_int_to_float(*ib.a, n, vp(ob.ptr), n - 1), "d_out")
    _invalid(_dbg().mpn_debug_int_to_float(*ib.a, 0, *ob.a))
    assert _is_sent(ob.read())


# ---- linear_dgrad_c8, the tower backward's form ----------------------------------------------------------------------------------------
def _run_prefix(g_rows, wpk, N, rows, K_launch, pitch):
    """the unmasked form (act null, scale 1) over `rows` rows at g_Mp = x_Mp = pitch -> dx [Kfull / 8][pitch][8]"""
    g_c8 = R.c8_pack(g_rows[:rows], pitch, lane_fill=SENT_F, row_fill=SENT_F)   # lanes n >= N and the rows beyond the launch's: never read

    def call():
        gb, wb, db = Buf(g_c8), Buf(wpk), Buf(_sent(Q.DG_KFULL // 8, pitch, 8))
        _ok(_dbg().mpn_debug_linear_dgrad_c8(*gb.a, pitch, rows, N, *wb.a, K_launch, *NULL, *db.a, pitch, 1.0))
        assert _same(gb.read(), g_c8) and _same(wb.read(), wpk), "an input was written"
        return (db.read(),)
    return twice(call)[0]


@pytest.mark.parametrize("N,PP,B", Q.DG_CASES)
def test_linear_dgrad_prefix_launch(dev, N, PP, B):
    Mp, Kf, Kc = Q.DG_MP, Q.DG_KFULL, Q.DG_K
    g, w, valid = Q.dgrad_inputs(N, PP, B)
    pitch, rows = PP * Mp, (PP - 1) * Mp + B
    tag = "N %d PP %d B %d" % (N, PP, B)
    g_nan, g_zero = g.copy(), g.copy()
    g_nan[~valid], g_zero[~valid] = np.nan, 0.0
    wide = R.lin_pack(w, 1, fill=SENT_F)                 # packed for Kfull columns; rows n >= N and pad lanes: never read
    ref = g.astype(F64) @ w.astype(F64)
    v = valid[:rows]

    def check(dx, K_launch, what):
        nch = Q.cdiv(K_launch, 8)
        assert _is_sent(dx[nch:]) and _is_sent(dx[:, rows:]), "a dx chunk >= K / 8 or a row beyond the launch's was written"
        return R.c8_unpack(dx[:nch], rows, nch * 8)
    d_nan = check(_run_prefix(g_nan, wide, N, rows, Kc, pitch), Kc, "stale NaN")
    assert np.isfinite(d_nan[v]).all(), "a stale row's NaN reached a valid row"
    assert np.isnan(d_nan[~v]).all()                     # the stale rows' own results: theirs alone
    _bits_acc("dgrad prefix launch == float64 " + tag, d_nan[v], ref[:rows][v][:, :Kc].astype(F32))
    d_zero = check(_run_prefix(g_zero, wide, N, rows, Kc, pitch), Kc, "stale zero")
    _bits_acc("dgrad prefix launch, stale rows NaN == zeroed " + tag, d_nan[v], d_zero[v])
    d_own = check(_run_prefix(g_nan, R.lin_pack(w[:, :Kc], 1, fill=SENT_F), N, rows, Kc, pitch), Kc, "own pack")
    _bits_acc("dgrad wide pack == a pack for K alone " + tag, d_nan[v], d_own[v])
    if (PP, B) == (4, 3):   # K = 44 on a pack whose last chunk is padded with +0.0 lanes: real lanes exact, the four pad lanes +-0
        d44 = check(_run_prefix(g_nan, Q.lin_pack_zero_pad(w[:, :44]), N, rows, 44, pitch), 44, "K 44")
        _bits_acc("dgrad K 44 real lanes == float64 " + tag, d44[v][:, :44], ref[:rows][v][:, :44].astype(F32))
        assert not d44[v][:, 44:].any() and np.isfinite(d44[v][:, 44:]).all(), "a pad lane of the last chunk is not +-0"
