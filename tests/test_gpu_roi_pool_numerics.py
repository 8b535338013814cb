"""The trunk-side ROI poolings and the L2 normalisation behind them (multipathnet_amd/csrc/dense.hip), one form at a time, against float64
and against NumPy restatements of the orders dense.hip documents: roi_pool_c8_kernel<LEVELS> (with arg-max), vmax_level_kernel +
roi_pool_c8_rmq_kernel, c8p_to_pixel_major_kernel + roi_pool_pm_kernel<0, LEVELS>, vmax_level_pm_kernel + roi_pool_pm_rmq_kernel<SS>,
l2norm_partial / _finish / _apply (l2norm_scale_c8, mul_const_c8), l2norm_finish_rows_kernel and l2norm_scale_rows_kernel.  Both flagship
pipelines and both training drivers push every number through this family; until now its forms were only compared with each other
(mpn_debug_roi_pool_rmq_mismatches: C <= 40, finite data, zeroed outputs, one pitch, no arg-max, no LEVELS, no normalising form).

The kernels are called through mpn_debug_roi_pool_form, mpn_debug_vmax_tables and mpn_debug_l2norm_c8 (debug flavour only): raw device
pointers in the kernels' own layouts, the product's host wrappers, an element count per caller-owned buffer.  Layouts, references, bounds
and input sets are tests/roi_pool_np.py's (checked on the CPU in tests/test_roi_pool_ref_cpu.py).

Common setup.  Every device buffer sits between two guard zones of 256 sentinel NaNs (0x7FA5A5A5) that must survive every launch.  Every
output is pre-filled with the sentinel: rows n >= N of every record, the scale vector beyond Mp and the arg-max beyond N * C * PH * PW must
keep it.  Halo and pitch padding of the feature planes hold 2^100 (finite, above every real value: `>` is blind to a NaN halo); the pad
lanes of a ragged last channel block hold +0, must come out +0 and must add nothing to a sum of squares.  Column 0 of the ROI table holds
NaN in the forms without LEVELS.  Every case runs twice on fresh buffers: the same bits.

Tiers.
  exact      pooled values of all four forms (and form 3 followed by mul_const_c8): equal to the float64 maximum bit for bit except between
             +0 and -0, the same NaN / +inf / -inf class, the arg-max equal; the range-max tables equal as values; the LEVELS map choice.
  bit-exact  the in-place normalisation of both orders and the scale vector against the fp32 restatement of the documented order
             (-ffp-contract=off; HIP's default sqrtf and division are correctly rounded on this build: the restatement uses IEEE ones and
             every case agrees in every bit, so no step had to be isolated).
  derived    the same against float64 inside tests/roi_pool_np.py's bound; ACC lines give the largest error / bound per family.

What the module found.  include/mpn.h says a pooling window ignores its NaNs, dense.h that the range-max forms give roi_pool_c8's output.
The direct kernels did; the two table builders and the two table readers selected with `b > a ? b : a`, which keeps a NaN `a`: a NaN at
the head of a row range (or of its power-of-two sub-range) poisoned the range.  On the MI355X, before the fix: [NaN, 5] over rows [0, 2)
gave -inf where the direct kernel gives 5, and [1, 3, NaN, 9] over rows [0, 4) gave the finite wrong value 3 instead of 9 (forms 1 and 3;
test_nan_examples, test_tables and every `edge` case of test_pooled failed).  The builders now select with `(b > a || a != a) ? b : a` and
the readers compare each of their two table values with the running maximum (`v > m`, the direct kernel's rule, at the old operation
count); results on NaN-free maps, the sign of zero included, are bit for bit what they were.  Also pinned as contract: a bin holding nothing above -inf
(only NaN and -inf) reports arg-max -1, like an empty one.

MEASURED on the MI355X (111 cases, 4.2 s; largest observed error / bound per family from the ACC lines; DESIGN.md section 13.10 has the
same table):
  fused in place (roi_pool_pm_rmq, normalize 1)        0.0136  (C 8, K 392); K = 392 / 784 / 1960 / 12936: 0.0136 / 0.0049 / 0.0026 / 0.0005
  fused scale vector (l2norm_scale_rows_kernel)        0.0061  (C 8, K 392); K = 12936: 0.0004
  l2norm_scale_c8 behind a pooling                     0.0168  (K 392); K = 12936: 0.0014
  l2norm_scale_c8 on its own                           0.2324  (one record, K 8); n_records 50 / 98 / 120 / 147: 0.039 / 0.020 / 0.009 / 0.012
  The device's bits are the restated order's in every case, the overflowing and the all-zero ones included.

Mutations tried on scratch copies of the debug library (MI355X; each in bounds by construction: the entry's own buffers carry slack
holding FLT_MAX, and test_l2norm_c8 allocates up to the next multiple of 49 records), with the first test that fails on each:
  roi_pool_pm_rmq_kernel's min(xb + j, we - 1) as xb + j                     test_pooled[3-1-1-1-edge-1-...]
  roi_pool_c8_rmq_kernel's min(xb + j, we - 1) as xb + j                     test_pooled[3-1-1-1-edge-1-...]
  k as the ceiling log2, pixel-major reader / C8P reader                     test_pooled[20-9-3-3-edge-0-...] each
  r1 from he - (1 << k) - 1, pixel-major reader / C8P reader                 test_pooled[3-1-1-1-edge-1-...] each
  vmax_level_kernel's y + step < H as <=                                     test_tables[8x2x37-edge-0]
  vmax_level_pm_kernel's y + step < H as <=                                  test_tables[8x2x37-edge-1]
  the ch < C guard dropped in roi_pool_pm_rmq_kernel                         test_normalize[3-1-1-130-neg-...] (the sum of squares)
  the n0 + roi < N store guard dropped in roi_pool_pm_rmq_kernel             test_pooled[3-1-1-1-edge-0-...] (a row n >= N written)
  roi_level_offset ignoring column 0                                         test_levels[0-0]
  roi_pool_c8_kernel's arg-max update on >=                                  test_pooled[8-2-37-1-quant-1-...]
  l2norm_partial_kernel's r1 without the min                                 test_l2norm_c8[1-1-8]
  l2norm_scale_rows_kernel writing 0 on the pad rows                         test_normalize[3-1-1-1-mixed-0-...]
None slipped through.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roi_pool_np as R  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENT = R.SENT
GUARD = 256
MPN_EINVAL = -1
cf, ci, cs, vp = C.c_float, C.c_int, C.c_size_t, C.c_void_p
ACC = {}


@functools.lru_cache(maxsize=None)
def _dbg():
    from multipathnet_amd import _lib
    lib = _lib.load("debug")
    b = [vp, cs]  # a buffer and its element count
    lib.mpn_debug_roi_pool_form.argtypes = [ci] + b + [ci, ci, ci, ci, cs] + b + [ci, ci, ci, ci, cf, ci, ci, ci, cf] + b + b + b
    lib.mpn_debug_vmax_tables.argtypes = [ci] + b + [ci, ci, ci] + b
    lib.mpn_debug_l2norm_c8.argtypes = b + [ci, ci, ci, cf, ci]
    return lib


def _ok(rc):
    assert rc == 0, (rc, _dbg().mpn_last_error().decode())


def _sent(n, dtype=F32):
    return np.full(n, SENT, np.uint32).view(dtype)


def _is_sent(a):
    return bool((np.ascontiguousarray(a).view(np.uint32) == SENT).all())


class Buf(object):
    """a device buffer between two guard zones of GUARD sentinel words; .a = (pointer, element count) as the entries take them"""

    def __init__(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.dtype in (np.float32, np.int32)
        self.shape, self.dtype, self.n = arr.shape, arr.dtype, arr.size
        host = np.full(self.n + 2 * GUARD, SENT, np.uint32)
        host[GUARD:GUARD + self.n] = arr.reshape(-1).view(np.uint32)
        self.host = host[GUARD:GUARD + self.n].copy()
        self.t = torch.from_numpy(host.view(np.int32)).to(torch.device("cuda", 0))
        self.ptr = self.t.data_ptr() + 4 * GUARD
        assert self.ptr % 16 == 0
        self.a = (vp(self.ptr), self.n)

    def at(self, off):
        return (vp(self.ptr + 4 * off), self.n - off)

    def read(self):
        torch.cuda.synchronize()
        h = self.t.cpu().numpy().view(np.uint32)
        assert (h[:GUARD] == SENT).all() and (h[GUARD + self.n:] == SENT).all(), "a launch wrote into a guard zone"
        return h[GUARD:GUARD + self.n].view(self.dtype).reshape(self.shape).copy()

    def unchanged(self):
        return np.array_equal(self.read().reshape(-1).view(np.uint32), self.host)


NULL = (None, 0)


def twice(call):
    """every case runs twice on fresh buffers: the same bits.  call() -> tuple of numpy arrays (or None)"""
    a, b = call(), call()
    for x, y in zip(a, b):
        assert (x is None and y is None) or np.array_equal(x.view(np.uint32), y.view(np.uint32)), "two runs differ"
    return a


def _table(rois, stride, region):
    """the device ROI table and the float offset of its base: [N, 5] with NaN in column 0, or the [N, 4, 5] Foveal table entered at `region`"""
    if stride == 5:
        t = rois.copy()
        t[:, 0] = np.nan
        return t.reshape(-1), 0
    return R.foveal_table(rois, region).reshape(-1), 5 * region


def _pool(form, fmap, C_, H, W, table, roi_off, stride, N, PH, PW, scale, rule, Mp, normalize=0, mul=1.0, argmax=False, scale_out=False, n_levels=0,
          level_stride=0):
    """one call of mpn_debug_roi_pool_form on fresh sentinel-filled outputs, twice -> (x flat, argmax or None, scale or None)"""
    mp = Mp or R.lin_mp(N)
    Cb, PP = R.cdiv(C_, 8), PH * PW

    def call():
        fb, rb = Buf(fmap), Buf(table)
        xb = Buf(_sent(Cb * PP * mp * 8))
        ab = Buf(_sent(N * C_ * PP + 64, np.int32)) if argmax else None
        sb = Buf(_sent(mp + 64)) if scale_out else None
        _ok(_dbg().mpn_debug_roi_pool_form(form, *fb.a, C_, H, W, n_levels, level_stride, *rb.at(roi_off), stride, N, PH, PW, scale, rule, Mp, normalize,
                                           mul, *xb.a, *(ab.a if ab else NULL), *(sb.a if sb else NULL)))
        assert fb.unchanged() and rb.unchanged(), "an input was written"
        return xb.read(), ab.read() if ab else None, sb.read() if sb else None
    return twice(call)


def _check_pooled(tag, x, C_, PP, mp, N, ref, mul=None):
    """x: the C8 matrix; ref float64 [N, C, PP].  Bits equal except between +-0, classes equal, pad lanes +0, rows >= N untouched."""
    a = R.c8_unpack(x, C_, PP, mp)
    assert _is_sent(a[N:]), tag + ": a row n >= N was written"
    assert (R.bits(a[:N, C_:]) == 0).all(), tag + ": a pad lane is not +0"
    got, want = a[:N, :C_], ref.astype(F32)
    assert np.array_equal(want.astype(F64), ref)
    if mul is not None:
        with np.errstate(all="ignore"):
            want = want * F32(mul)
    assert not np.isnan(want).any()
    assert np.array_equal(R.value_class(got), R.value_class(want)), tag + ": NaN / inf classes differ"
    assert np.array_equal(got, want), (tag, int((got != want).sum()), got[got != want][:4], want[got != want][:4])
    nz = want != 0
    assert np.array_equal(R.bits(got)[nz], R.bits(want)[nz]), tag


def _acc(tag, got, ref, K, ops):
    bound = R.l2norm_bound(ref, K, ops)
    err = np.abs(np.asarray(got, F64) - ref)
    assert np.isfinite(err).all(), tag + ": a NaN or inf in the result"  # (max() and `<=` are both blind to a NaN)
    nz = bound > 0
    assert (err[~nz] == 0).all(), tag
    ratio = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    ACC[tag] = max(ACC.get(tag, 0.0), ratio)
    print("ACC %-24s K = %6d  err / bound = %.4f" % (tag, K, ratio))
    assert ratio <= 1.0, tag
    return ratio


def _same_bits(got, want):
    return np.array_equal(R.bits(got), R.bits(want))


# ---- pooled values, all four forms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.pool_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_pooled(dev, case):
    C_, H, W, N, kind, rule, scale, Mp, stride, region, PH, PW = case
    feat, rois, ref = R.pool_inputs(C_, H, W, N, kind, rule, scale, PH, PW)
    fmap = R.c8p_pack(feat)
    table, off = _table(rois, stride, region)
    mp, PP = Mp or R.lin_mp(N), PH * PW
    ref = ref.reshape(N, C_, PP)
    arg_ref = R.roi_argmax(feat, rois, PH, PW, scale, rule)
    for form in (0, 1, 2, 3):
        x, arg, _ = _pool(form, fmap, C_, H, W, table, off, stride, N, PH, PW, scale, rule, Mp, argmax=(form == 0))
        _check_pooled("form %d" % form, x, C_, PP, mp, N, ref)
        if form == 0:
            assert _is_sent(arg[N * C_ * PP:]), "the arg-max beyond N * C * PH * PW was written"
            assert np.array_equal(arg[:N * C_ * PP].reshape(arg_ref.shape), arg_ref)
            x2, _, _ = _pool(0, fmap, C_, H, W, table, off, stride, N, PH, PW, scale, rule, Mp)  # without the arg-max: the same values
            assert np.array_equal(x2.view(np.uint32), x.view(np.uint32))
    x, _, _ = _pool(3, fmap, C_, H, W, table, off, stride, N, PH, PW, scale, rule, Mp, normalize=0, mul=1.7)  # + mul_const_c8
    _check_pooled("form 3 x 1.7", x, C_, PP, mp, N, ref, mul=1.7)


COLUMNS = (([np.nan, 5.0], 5.0), ([1.0, 3.0, np.nan, 9.0], 9.0), ([np.nan, np.nan, -2.0], -2.0), ([np.nan, np.nan], -np.inf))


@pytest.mark.parametrize("col,want", COLUMNS, ids=("nan5", "13nan9", "nannan-2", "nannan"))
def test_nan_examples(dev, col, want):
    """one column, one bin over all of it: a window ignores its NaNs in every form, and gives -inf only when it holds nothing else"""
    H = len(col)
    feat = np.array(col, F32).reshape(1, H, 1)
    rois = np.array([[1, 1, 1, 1, H]], F32)
    table, off = _table(rois, 5, 0)
    got = []
    for form in (0, 1, 2, 3):
        x, _, _ = _pool(form, R.c8p_pack(feat), 1, H, 1, table, off, 5, 1, 1, 1, 1.0, 0, 0)
        got.append(float(R.c8_unpack(x, 1, 1, 128)[0, 0, 0]))
    print("NAN column %s: forms 0..3 give %s, float64 %s" % (col, got, want))
    assert got == [want] * 4


# ---- the range-max tables -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pm", (0, 1))
@pytest.mark.parametrize("kind", ("edge", "quant"))
@pytest.mark.parametrize("shape", R.MAPS, ids=lambda s: "x".join(map(str, s)))
def test_tables(dev, shape, kind, pm):
    C_, H, W = shape
    feat = R.make_map(kind, C_, H, W, 7)
    L, Cb = R.vmax_levels(H), R.cdiv(C_, 8)
    T = R.vmax_tables64(feat)
    ae, pe = R.act_elems(C_, H, W), H * W * Cb * 8
    n_out = pe * (L + 1) if pm else ae * L

    def call():
        fb, tb = Buf(R.c8p_pack(feat)), Buf(_sent(n_out + 4))
        _ok(_dbg().mpn_debug_vmax_tables(pm, *fb.a, C_, H, W, *tb.a))
        assert fb.unchanged()
        return (tb.read(),)
    out, = twice(call)
    assert _is_sent(out[n_out:])
    for k in range(0 if pm else 1, L + 1):
        if pm:
            lv = R.pm_unpack(out[k * pe:(k + 1) * pe], C_, H, W)
        else:
            raw = out[(k - 1) * ae:k * ae].reshape(Cb, R.act_hp(H), R.act_wp(W), 8)
            halo = np.ones(raw.shape, bool)
            halo[:, 1:H + 1, 1:W + 1, :] = False
            assert (raw[halo] == np.finfo(F32).max).all(), "a table builder wrote outside the interior"
            lv = R.c8p_unpack(raw, C_, H, W)
        assert (R.bits(lv[C_:]) == 0).all(), "a pad lane of level %d is not +0" % k
        got, want = lv[:C_].astype(F64), T[k]
        assert np.array_equal(R.value_class(got), R.value_class(want)), "level %d: classes" % k
        ok = ~np.isnan(want)
        assert np.array_equal(got[ok], want[ok]), "level %d" % k


# ---- LEVELS ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", (0, 1))
@pytest.mark.parametrize("form", (0, 2))
def test_levels(dev, form, rule):
    """a ROI reads the map its column 0 names: 1 .. n the 1-based level, 2.7 truncates to level 2, and 0, n + 1, -1 and NaN read level 1
    (roi_level_offset).  The three maps differ by +8 / +16 / +0, so two of every three misreads would win."""
    C_, H, W, n_levels, scale, Mp = 20, 9, 3, 3, 0.25, 16
    col0 = np.array([0, n_levels + 1, 2.7, -1, np.nan, 1, 2, 3], F32)
    level = [0, 0, 1, 0, 0, 0, 1, 2]
    N = len(col0)
    maps = [R.make_map("mixed", C_, H, W, 20 + l) + F32(8 * ((l + 1) % 3)) for l in range(n_levels)]
    rois = R.make_rois(N, H, W, scale, 2, rule)
    ae = R.act_elems(C_, H, W)
    stride = ae + 64
    fmap = _sent((n_levels - 1) * stride + ae)
    for l in range(n_levels):
        fmap[l * stride:l * stride + ae] = R.c8p_pack(maps[l]).reshape(-1)
    table = rois.copy()
    table[:, 0] = col0
    ref = np.concatenate([R.roi_pool64(maps[level[n]], rois[n:n + 1], 7, 7, scale, rule) for n in range(N)]).reshape(N, C_, 49)
    x, arg, _ = _pool(form, fmap, C_, H, W, table.reshape(-1), 0, 5, N, 7, 7, scale, rule, Mp, argmax=(form == 0), n_levels=n_levels, level_stride=stride)
    _check_pooled("levels form %d" % form, x, C_, 49, Mp, N, ref)
    if form == 0:
        arg_ref = np.concatenate([R.roi_argmax(maps[level[n]], rois[n:n + 1], 7, 7, scale, rule) for n in range(N)])
        assert np.array_equal(arg[:N * C_ * 49].reshape(arg_ref.shape), arg_ref) and _is_sent(arg[N * C_ * 49:])


# ---- the normalising forms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.norm_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_normalize(dev, case):
    C_, H, W, N, kind, rule, scale, Mp, mul = case
    feat, rois, ref = R.pool_inputs(C_, H, W, N, kind, rule, scale, 7, 7, True)
    fmap = R.c8p_pack(feat)
    table, off = _table(rois, 5, 0)
    mp, Cb = Mp or R.lin_mp(N), R.cdiv(C_, 8)
    p = R.pooled_padded(ref, C_)            # [N, Cb * 8, 49], pad lanes +0
    emu_y, emu_s = R.l2norm_fused_f32(p, mul)
    K = Cb * 8 * 49
    finite = kind != "huge"
    y64, s64 = R.l2norm64(p.reshape(N, -1), mul)
    # in place
    x, _, _ = _pool(3, fmap, C_, H, W, table, off, 5, N, 7, 7, scale, rule, Mp, normalize=1, mul=mul)
    a = R.c8_unpack(x, C_, 49, mp)
    assert _is_sent(a[N:])
    assert _same_bits(a[:N], emu_y), "in place: not the documented order's bits"
    if finite:
        _acc("fused in place", a[:N].reshape(N, -1), y64, K, 2)
    # the scale vector; the matrix stays as pooled
    x, _, s = _pool(3, fmap, C_, H, W, table, off, 5, N, 7, 7, scale, rule, Mp, normalize=1, mul=mul, scale_out=True)
    a = R.c8_unpack(x, C_, 49, mp)
    assert _is_sent(a[N:]) and _same_bits(a[:N], p)
    assert _same_bits(s[:N], emu_s), "scale: not the documented order's bits"
    assert (R.bits(s[N:mp]) == R.bits(F32(1.0))).all() and _is_sent(s[mp:])
    if finite:
        _acc("fused scale", s[:N], s64, K, 1)
    # l2norm_scale_c8 on the same pooled matrix
    c8 = R.c8_pack(p, mp)

    def call():
        xb = Buf(c8)
        _ok(_dbg().mpn_debug_l2norm_c8(*xb.a, Cb * 49, mp, N, mul, 1))
        return (xb.read(),)
    y, = twice(call)
    assert _same_bits(y, R.l2norm_c8_f32(c8, N, mul)), "l2norm_scale_c8: not the documented order's bits"
    if finite:
        _acc("l2norm_scale_c8", R.c8_unpack(y, C_, 49, mp)[:N].reshape(N, -1), y64, K, 2)
    zero = ~(p != 0).any(axis=(1, 2))
    assert zero[0] or rule == 1
    if zero.any():  # an all-zero ROI: zeros and a finite scale
        assert (R.bits(a[:N][zero]) == 0).all() and np.isfinite(s[:N][zero]).all() and (s[:N][zero] > 0).all()


@pytest.mark.parametrize("nrec,N,Mp", R.L2_CASES)
def test_l2norm_c8(dev, nrec, N, Mp):
    """l2norm_scale_c8 and mul_const_c8 on their own, n_records on and off a multiple of the 49-record group; the records past n_records up
    to the next multiple of 49 hold the sentinel and keep it"""
    x = R.l2_inputs(nrec, N, Mp)
    mp = x.shape[1]
    full = np.concatenate([x, _sent((R.round_up(nrec, 49) - nrec) * mp * 8).reshape(-1, mp, 8)])

    def run(mul, normalize):
        def call():
            xb = Buf(full)
            _ok(_dbg().mpn_debug_l2norm_c8(*xb.a, nrec, mp, N, mul, normalize))
            return (xb.read(),)
        y, = twice(call)
        assert _is_sent(y[nrec:]) and _is_sent(y[:nrec, N:, :])
        return y[:nrec]
    y = run(0.37, 1)
    assert _same_bits(y, R.l2norm_c8_f32(x, N, 0.37))
    v = x[:, :N, :].transpose(1, 0, 2).reshape(N, -1)
    _acc("l2norm_scale_c8", y[:, :N, :].transpose(1, 0, 2).reshape(N, -1), R.l2norm64(v, 0.37)[0], nrec * 8, 2)
    assert _same_bits(run(1.7, 0)[:, :N, :], x[:, :N, :] * F32(1.7))
    assert _same_bits(run(1.0, 0), x)


def test_sqrt_and_division_are_correctly_rounded(dev):
    """the step the bit-exact tier leans on, isolated: rows holding one power-of-two element v have the sum v^2 exactly, so d is the fp32
    sqrtf(v^2 + 1e-10f) and the scale the fp32 quotient mul / d — compared with IEEE sqrt and division"""
    N, mp = 64, 128
    x = np.zeros((1, mp, 8), F32)
    v = np.exp2(np.arange(N) - 40.0).astype(F32)
    x[0, :N, 3] = v
    x[0, N:, :] = R.SENT_F

    def call():
        xb = Buf(x)
        _ok(_dbg().mpn_debug_l2norm_c8(*xb.a, 1, mp, N, 3.0, 1))
        return (xb.read(),)
    y, = twice(call)
    with np.errstate(all="ignore"):
        want = (v / np.sqrt(v * v + R.EPS32)) * F32(3.0)
    assert _same_bits(y[0, :N, 3], want) and _is_sent(y[0, N:, :])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    """each entry refuses a buffer one element short, before anything is launched"""
    C_, H, W, N = 20, 9, 3, 5
    feat, rois, _ = R.pool_inputs(C_, H, W, N, "mixed", 0, 0.25)
    table, _ = _table(rois, 5, 0)
    mp = R.lin_mp(N)
    lib = _dbg()
    for form, short in ((0, "feat"), (1, "rois"), (2, "x"), (0, "arg"), (3, "scale"), (3, "x")):
        fb, rb, xb = Buf(R.c8p_pack(feat)), Buf(table), Buf(_sent(3 * 49 * mp * 8))
        ab = Buf(_sent(N * C_ * 49, np.int32)) if form == 0 else None
        sb = Buf(_sent(mp)) if form == 3 else None
        cut = lambda b, name: (b.a[0], b.n - (1 if short == name else 0))  # noqa: E731
        rc = lib.mpn_debug_roi_pool_form(form, *cut(fb, "feat"), C_, H, W, 0, 0, *cut(rb, "rois"), 5, N, 7, 7, 0.25, 0, 0, 1 if form == 3 else 0, 1.0,
                                         *cut(xb, "x"), *(cut(ab, "arg") if ab else NULL), *(cut(sb, "scale") if sb else NULL))
        assert rc == MPN_EINVAL, (form, short, rc)
        assert "footprint" in lib.mpn_last_error().decode()
        assert _is_sent(xb.read()) and (ab is None or _is_sent(ab.read())) and (sb is None or _is_sent(sb.read()))
    ae, pe, L = R.act_elems(C_, H, W), H * W * 24, R.vmax_levels(H)
    for pm, short in ((1, "feat"), (0, "tab"), (1, "tab")):
        fb, tb = Buf(R.c8p_pack(feat)), Buf(_sent(pe * (L + 1) if pm else ae * L))
        rc = lib.mpn_debug_vmax_tables(pm, fb.a[0], fb.n - (short == "feat"), C_, H, W, tb.a[0], tb.n - (short == "tab"))
        assert rc == MPN_EINVAL and _is_sent(tb.read())
    xb = Buf(_sent(50 * 8 * 8))
    assert lib.mpn_debug_l2norm_c8(xb.a[0], xb.n - 1, 50, 8, 5, 2.0, 1) == MPN_EINVAL and _is_sent(xb.read())
    assert lib.mpn_debug_l2norm_c8(xb.a[0], xb.n - 1, 50, 8, 5, 2.0, 0) == MPN_EINVAL and _is_sent(xb.read())


def test_zz_acc_summary(dev):
    """the largest error / bound of each family over the module (run after the tests that fill it)"""
    for tag in sorted(ACC):
        print("ACC-MAX %-24s %.4f" % (tag, ACC[tag]))
    assert all(v <= 1.0 for v in ACC.values())
