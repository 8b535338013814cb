"""The detection head's score and box kernels (boxes.hip, pipeline.hip, nms.hip's bbox_vote), one launch at a time, against float64 restatements.

The four kernels that only the pipelines launch (head_softmax_kernel, integral_softmax_mean_kernel, head_decode_kernel, augment_merge_kernel) are
reached through mpn_debug_head_post (debug flavour only), which calls the pipeline's own static launchers; launch_bbox_decode's fused clamp through
mpn_debug_bbox_decode_clamp; everything else through the product library's entries.  Every output buffer first holds a sentinel NaN (rows past M
and columns outside the written range must keep it), every entry runs twice and must give the same bits, and every device buffer is a torch
allocation (16-byte aligned).  The references are tests/boxes_np.py's, themselves checked against the CPU oracle in tests/test_boxes_ref_cpu.py on
the shape lists used here.

Softmax bound.  d = fl32(x - max) is part of the documented order and exactly reproducible, so the reference is float64 exp(d) / sum exp(d) on
that d (against a float64 subtraction the fp32 chain is off by the input's conditioning, about 66 * 2^-24 at sigma = 40: not the kernel's).  In
units of 2^-24, relative, per element: expf is within 1 ulp = 2 in the numerator; every summand carries the same 2; the sum is taken as
ceil(C / 64) serial additions per lane and 6 butterfly steps (6 + ceil(C / 64) roundings, all terms positive); the quotient 1:
11 + ceil(C / 64).  The integral kernel adds K - 1 sums in k order, fl32(1 / K) and the product: K + 1 more.  Elements whose float64 value is
below 2^-126 are outside the ratio and must lie in [0, 2^-125]; at sigma = 1 and 5 there is none; at sigma = 40 each row's maximum must get a
value in (0, 1] and the row must sum to 1 within the bound.

Decode bound (first order, absolute, units of 2^-24), for o = xtc -+ hw with xc = (x1 + x2) * 0.5, w = x2 - x1, xtc = xc + d * w,
hw = expf(dw) * w * 0.5: |x1 + x2| (the sum; the halving is exact) + 2 |d w| (w, the product) + |xtc| + 4 |hw| (expf 2, w 1, the product 1) + |o|;
with BBoxNorm a normed delta carries |d s| + |d s + m| of its own, which reaches o through |w| (dx, dy) or through |hw| (dw, dh).

Vote bound: tests/boxes_np.py vote().  Image scale bound: tests/boxes_np.py scale_pass_bound().

What the module found.  utils.convertFrom passed `bbox.contiguous()` and `y.contiguous()` as two temporaries of one call expression: the first is
freed as soon as its pointer is taken, the caching allocator hands the same block to the second, and the kernel decodes the deltas against
themselves.  Any caller with two column views (what utils.lua's narrow() gives) got garbage; the pointer-contract test met it through the copy that
a misaligned view now takes.  Both callers keep their copies in named locals until the launch is enqueued
(test_utils_decode_copies_a_misaligned_view).  The kernels themselves met every check.  Three of the issue's mutations cannot be observed and are
not errors of the suite: `<=` for `<` in a clamp returns the bound for a value equal to the bound, the same bits; image_scale's `i1 > i0` guard
is never false in the down-scaling branch (scale > 1, so s1 - s0 > 1); and a constant image is reproduced bit for bit only where the constant is a
power of two (tests/test_boxes_ref_cpu.py).

MEASURED on the MI355X (max relative error over all cases of a regime against float64, in units of 2^-24; "oracle" is the CPU oracle's serial
fp32 chain on the same inputs, glibc expf):
  softmax_kernel       sigma 1: 3.47 (C = 63)   sigma 5: 5.56 (C = 65)   sigma 40: 3.82 (C = 129); oracle 0-19.8 / 0-48.6 / 0-4.5 (largest at C = 1000)
  head_softmax_kernel  sigma 1: 3.47            sigma 5: 5.56            sigma 40: 3.82;           oracle 0-13.8 / 0-22.7 / 0-4.2 (C <= 256)
  integral kernel      sigma 1: 4.15 (K = 6)    sigma 5: 7.62 (K = 6)    sigma 40: 4.87 (K = 8)    against a bound of 12 + K + 1 .. 15 + K + 1
  device / oracle per case at C >= 128: 0.15-1.23 (sigma 1), 0.07-1.38 (sigma 5), 0.67-2.19 (sigma 40, where up to 87 % of a row lies below 2^-126
  and the oracle chain is itself only 4 units): the lane-strided tree stays near 3-6 units where the serial chain grows with C.
  No case came within a factor of two of the bound, so expf was not measured on its own.
  decode: largest error / derived bound 0.727 (sigma 0.3), 0.707 (sigma 2).  bbox_vote: 0.570 (m = 256) over the single-table cases.
  The module's wall time is 6 s.

Mutations tried on scratch copies of the libraries (MI355X), each with the first test that fails on it:
  head_softmax_kernel rows at stride C, not ld                      test_softmax_vs_float64[head-1.0]
  head_softmax_kernel's max loop from lane + 64                     test_softmax_vs_float64[head-1.0]
  integral kernel's accv indexed q & 1                              test_softmax_vs_float64[integral-1.0]
  integral kernel multiplying by 1 / K inside the k loop            test_integral_equals_fp32_mean_of_head_softmaxes[6]
  head_decode_kernel ignoring col0                                  test_decode_tier1_bit_equal[1]
  head_decode_kernel applying the norm after the decode             test_decode_tier1_bit_equal[1]
  augment_merge_kernel flipping b0 into o0                          test_augment_merge_bit_equal[1-1]
  bbox_vote (both kernels) staging a full tile on the last tile     test_bbox_vote_bit_equal_and_vs_float64[1]
  bbox_vote_kernel's act as i <= n_nms                              test_bbox_vote_bit_equal_and_vs_float64[1]
  bbox_vote_batched_kernel's pow on every column                    test_bbox_vote_batched[1-0.5]
  select_scored_kernel's base_s advanced before the writes          test_select_scored_bit_equal[2]
The last-tile and base_s mutants read or write past the tables; the 256 rows after a scored table and the slab after the last class that the tests
allocate (and check) keep those accesses inside the tests' own buffers.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_np as A  # noqa: E402
import boxes_np as R  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64, U = np.float32, np.float64, R.U
SENT = 0x7FA5A5A5
MPN_EINVAL = -1
HEAD_SOFTMAX, INTEGRAL, HEAD_DECODE, MERGE = 0, 1, 2, 3
MEAN4, STD4 = (0.0, 0.01, -0.02, 0.03), (0.1, 0.1, 0.2, 0.2)
MEAN4_T1 = (0.02, 0.01, 0.0, 0.0)  # tier 1: the normed dw, dh stay exactly 0
cf, ci, cs = C.c_float, C.c_int, C.c_size_t


def _prod():
    from multipathnet_amd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _dbg():
    from multipathnet_amd import _lib
    lib = _lib.load("debug")
    vp = C.c_void_p
    f4 = C.POINTER(C.c_float * 4)
    lib.mpn_debug_head_post.argtypes = [ci, vp, vp, ci, ci, ci, ci, ci, f4, f4, ci, cf, cf, vp, vp, vp]
    lib.mpn_debug_bbox_decode_clamp.argtypes = [vp, vp, ci, ci, vp, ci, cf, cf, vp]
    return lib


def _err(lib):
    return lib.mpn_last_error().decode()


def _ok(lib, rc):
    assert rc == 0, (rc, _err(lib))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(torch.device("cuda", 0))


def _sent(*shape):
    return torch.full(shape, SENT, dtype=torch.int32, device=torch.device("cuda", 0)).view(torch.float32)


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _is_sent(a):
    return bool((_bits(a) == SENT).all())


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _same_nanpos(got, ref):
    """bit equality where the reference is a number; a NaN wherever it has one (the x86 and the device default NaNs differ in sign)"""
    got, ref = np.asarray(got, F32), np.asarray(ref, F32)
    n = np.isnan(ref)
    return np.array_equal(np.isnan(got), n) and np.array_equal(_bits(got)[~n], _bits(ref)[~n])


def twice(call):
    """every entry runs twice: the same bits.  call() -> tuple of numpy arrays"""
    a, b = call(), call()
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), "two runs differ"
    return a


# ---- softmax ---------------------------------------------------------------------------------------------------------------------------
def run_softmax(kernel, x, M, C_, K=1, ld=None, pad_rows=3):
    """x: [M, C] (forward, head) or [M, K*C] (integral) fp32 -> the whole output buffer [M + pad_rows, C]"""
    def call():
        out = _sent(M + pad_rows, C_)
        if kernel == "forward":
            lib, xd = _prod(), _dev(x)
            _ok(lib, lib.mpn_softmax_forward(_p(xd), M, C_, _p(out), None))
        elif kernel == "head":
            lib = _dbg()
            h = np.full((M, ld), 1e30, F32)  # a read past column C wins the max
            h[:, :C_] = x
            xd = _dev(h)
            _ok(lib, lib.mpn_debug_head_post(HEAD_SOFTMAX, _p(xd), None, ld, 0, M, C_, 0, None, None, 0, 0.0, 0.0, None, _p(out), None))
        else:
            lib, xd = _dbg(), _dev(x)
            _ok(lib, lib.mpn_debug_head_post(INTEGRAL, _p(xd), None, 0, 0, M, C_, K, None, None, 0, 0.0, 0.0, None, _p(out), None))
        return (_np(out),)
    buf = twice(call)[0]
    assert _is_sent(buf[M:]), "wrote rows past M"
    return buf[:M]


def _softmax_variants(kernel, C_):
    if kernel == "forward":
        return [dict()]
    if kernel == "head":
        return [dict(ld=C_), dict(ld=5 * C_), dict(ld=5 * C_ + 3)]
    return [dict(K=K) for K in R.SOFTMAX_K]


def _rel_err(got, ref):
    ok = ref >= R.TINY
    return ok, np.abs(got.astype(F64) - ref)[ok] / ref[ok]


@pytest.mark.parametrize("sigma", R.SOFTMAX_SIGMA)
@pytest.mark.parametrize("kernel", ["forward", "head", "integral"])
def test_softmax_vs_float64(O, dev, kernel, sigma):
    worst, worst_case, chain, small_frac = 0.0, None, [], 0.0
    ratio_big = []
    for C_ in (R.SOFTMAX_C_FREE if kernel == "forward" else R.SOFTMAX_C):
        for M in R.SOFTMAX_M:
            for v in _softmax_variants(kernel, C_):
                K = v.get("K", 1)
                rng = np.random.default_rng([M, C_, K, int(sigma)])
                x = R.logits(rng, M, K * C_, sigma)
                got = run_softmax(kernel, x, M, C_, **v)
                ref = R.softmax_mean(x.reshape(M, K, C_)) if kernel == "integral" else R.softmax(x)
                bound = R.softmax_bound(C_, K if kernel == "integral" else None)
                ok, rel = _rel_err(got, ref)
                assert (got[~ok] >= 0).all() and (got[~ok] <= 2.0 ** -125).all()
                if sigma < 40:
                    assert ok.all()
                else:
                    small_frac = max(small_frac, 1 - ok.mean())
                    top = got[np.arange(M), np.argmax(ref, 1)]
                    assert (top > 0).all() and (top <= 1).all()
                    assert np.abs(got.astype(F64).sum(1) - 1).max() <= bound
                e = float(rel.max()) if rel.size else 0.0
                if e > worst:
                    worst, worst_case = e, (M, C_, v)
                if kernel != "integral":
                    orc_e = _rel_err(O.softmax(x), ref)[1]
                    oe = float(orc_e.max()) if orc_e.size else 0.0
                    chain.append(oe / U)
                    if C_ >= 128 and oe > 0:
                        ratio_big.append(e / oe)
                assert e <= bound, (kernel, sigma, M, C_, v, e / U, bound / U)
    print("\nMEASURED softmax %s sigma=%g: max rel err %.2f u at %s (bound %s u)%s%s%s" % (
        kernel, sigma, worst / U, worst_case, "11+ceil(C/64)" + ("+K+1" if kernel == "integral" else ""),
        "; oracle chain %.2f-%.2f u" % (min(chain), max(chain)) if chain else "",
        "; device/oracle at C>=128: %.2f-%.2f" % (min(ratio_big), max(ratio_big)) if ratio_big else "",
        "; below 2^-126: up to %.0f %%" % (100 * small_frac) if sigma >= 40 else ""))


@pytest.mark.parametrize("kernel", ["forward", "head", "integral"])
def test_softmax_edge_rows(O, dev, kernel):
    inf, nan = np.inf, np.nan
    for C_ in (1, 2, 21, 64, 129, 256):
        base = R.logits(np.random.default_rng(C_), 1, C_, 1.0)[0]
        rows = [np.full(C_, 0.75, F32), base.copy(), base.copy(), np.full(C_, -inf, F32), base.copy(), base.copy(), base.copy()]
        rows[1][C_ // 2] = inf
        rows[2][C_ - 1] = -inf
        rows[4][0] = nan
        rows[5][0], rows[5][C_ - 1] = 3e38, -3e38
        x = np.stack(rows).astype(F32)
        M = x.shape[0]
        K = 2 if kernel == "integral" else 1
        if K == 2:  # the edge values in classifier 0, plain logits in classifier 1
            x = np.concatenate([x, R.logits(np.random.default_rng(C_ + 1), M, C_, 1.0)], 1)
            x[0, C_:] = 0.75
        got = run_softmax(kernel, x, M, C_, **(dict(K=2) if K == 2 else dict(ld=5 * C_ + 3) if kernel == "head" else {}))
        ref = R.softmax_mean(x.reshape(M, K, C_)) if K == 2 else R.softmax(x)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (kernel, C_)
        if K == 1:
            assert np.array_equal(np.isnan(O.softmax(x)), np.isnan(ref))  # the oracle's rule is the float64 rule
        n = ~np.isnan(ref)
        bound = R.softmax_bound(C_, K if K == 2 else None)
        assert (np.abs(got.astype(F64) - ref)[n] <= bound * ref[n] + 2.0 ** -125).all(), (kernel, C_)
        if C_ > 1:
            assert np.isnan(got[1]).all() and np.isnan(got[3]).all() and np.isnan(got[4]).all()  # inf - inf and NaN poison the row's sum
            assert got[5, C_ - 1] == (0 if K == 1 else got[5, C_ - 1]) and np.isfinite(got[5]).all() and np.isfinite(got[6]).all()
            if K == 1:
                assert got[2, C_ - 1] == 0  # one -inf: exactly 0 there
        if C_ & (C_ - 1) == 0:
            assert (got[0] == F32(1.0 / C_)).all()  # all-equal logits: exactly 1 / C where that is a float


def test_integral_k1_equals_head_softmax(dev):
    for C_ in R.SOFTMAX_C:
        for M in (5, 37):
            x = R.logits(np.random.default_rng([C_, M]), M, C_, 5.0)
            assert _same(run_softmax("integral", x, M, C_, K=1), run_softmax("head", x, M, C_, ld=C_)), (M, C_)


@pytest.mark.parametrize("K", R.SOFTMAX_K)
def test_integral_equals_fp32_mean_of_head_softmaxes(dev, K):
    """the documented order: each classifier's softmax as head_softmax_kernel computes it, summed in k order, then * fl32(1 / K) once"""
    for C_ in (2, 21, 65, 129, 256):
        M = 5
        x = R.logits(np.random.default_rng([C_, K, 3]), M, K * C_, 5.0)
        p = np.stack([run_softmax("head", np.ascontiguousarray(x[:, k * C_:(k + 1) * C_]), M, C_, ld=C_) for k in range(K)], 1)  # [M, K, C]
        assert _same(run_softmax("integral", x, M, C_, K=K), R.mean_over_k_f32(p)), (K, C_)


def test_head_post_refusals(dev):
    lib = _dbg()
    out, x = _sent(8, 300), _dev(np.zeros((8, 2400), F32))
    call = lambda which, M, C_, K, ld=2400: lib.mpn_debug_head_post(which, _p(x), _p(x), ld, 0, M, C_, K, None, None, 0, 0.0, 0.0, _p(out), _p(out), None)
    assert call(INTEGRAL, 4, 257, 1) == MPN_EINVAL and "C <= 256" in _err(lib)
    assert call(INTEGRAL, 4, 256, 1) == 0
    out = _sent(8, 300)
    for which in (HEAD_SOFTMAX, INTEGRAL, HEAD_DECODE, MERGE):
        assert call(which, 4, 0, 1) == MPN_EINVAL and call(which, -1, 4, 1) == MPN_EINVAL
        assert call(which, 0, 4, 1) == 0  # M = 0: nothing launched
    assert call(INTEGRAL, 4, 4, 0) == MPN_EINVAL
    assert call(HEAD_SOFTMAX, 4, 8, 1, ld=7) == MPN_EINVAL and call(HEAD_DECODE, 4, 8, 1, ld=31) == MPN_EINVAL
    assert _is_sent(_np(out))


# ---- decode ----------------------------------------------------------------------------------------------------------------------------
HEAD_LAYOUTS = ("5C", "4C", "5C+3")


def _layout(name, C_):
    return {"5C": (5 * C_, C_), "4C": (4 * C_, 0), "5C+3": (5 * C_ + 3, C_ + 1)}[name]


def run_decode(entry, boxes, deltas, N, C_, clamp=0, W=1000.0, H=600.0, layout="5C", norm=None, raw=False, pad_rows=2):
    """entry: "public" (mpn_bbox_decode), "fused" (launch_bbox_decode with its clamp argument), "head" (head_decode_kernel).
    Returns (out [N, 4C], raw [N, 4C] or None)."""
    def call():
        out = _sent(N + pad_rows, 4 * C_)
        rawd = _sent(N + pad_rows, 4 * C_) if raw else None
        bd = _dev(boxes)
        if entry == "head":
            lib = _dbg()
            ld, col0 = _layout(layout, C_)
            h = np.full((N, ld), 1e30, F32)
            h[:, col0:col0 + 4 * C_] = deltas
            hd = _dev(h)
            m4 = (C.c_float * 4)(*norm[0]) if norm else None
            s4 = (C.c_float * 4)(*norm[1]) if norm else None
            _ok(lib, lib.mpn_debug_head_post(HEAD_DECODE, _p(hd), _p(bd), ld, col0, N, C_, 0, m4, s4, clamp, W, H, _p(rawd), _p(out), None))
        else:
            dd = _dev(deltas)
            if entry == "public":
                assert not clamp
                lib = _prod()
                _ok(lib, lib.mpn_bbox_decode(_p(bd), _p(dd), N, C_, _p(out), None))
            else:
                lib = _dbg()
                _ok(lib, lib.mpn_debug_bbox_decode_clamp(_p(bd), _p(dd), N, C_, _p(out), clamp, W, H, None))
        return (_np(out),) + ((_np(rawd),) if raw else ())
    res = twice(call)
    for b in res:
        assert _is_sent(b[N:]), "wrote rows past N"
    return res[0][:N], (res[1][:N] if raw else None)


def _decode_cases():
    """(entry, kwargs): the public entry, the fused clamp on and off, and the head kernel over layouts x norm x raw x clamp (each option in
    at least one case with every layout)"""
    cases = [("public", {}), ("fused", dict(clamp=0)), ("fused", dict(clamp=1))]
    for i, lay in enumerate(HEAD_LAYOUTS):
        for norm in (False, True):
            for raw in (False, True):
                cases.append(("head", dict(layout=lay, norm=norm, raw=raw, clamp=(i + norm + raw) % 2)))
    return cases


def _deltas(rng, N, C_, sigma, tier1=False):
    d = (rng.standard_normal((N, 4 * C_)) * sigma).astype(F32)
    if tier1:
        d.reshape(N, C_, 4)[..., 2:] = 0
    return d


@pytest.mark.parametrize("C_", R.DECODE_C)
def test_decode_tier1_bit_equal(O, dev, C_):
    """dw = dh = 0: expf is exactly 1, so the whole chain is bit-equal to the oracle's; pins indexing, operation order and the clamp"""
    for N in R.DECODE_N:
        rng = np.random.default_rng([N, C_])
        b = R.rois(rng, N)
        b[::3] += F32(450)  # a third of the boxes reach past the image: the clamp has work on both sides
        b[1::3] -= F32(450)
        d = _deltas(rng, N, C_, 0.5, tier1=True)
        for entry, kw in _decode_cases():
            kw = dict(kw)
            norm = (MEAN4_T1, STD4) if kw.pop("norm", False) else None
            got, raw = run_decode(entry, b, d, N, C_, norm=norm, **kw)
            dn = O.bbox_norm(d, *norm) if norm else d
            exp = O.bbox_decode(b, dn)
            if kw.get("clamp"):
                exp = O.clamp_boxes(exp, 1000, 600)
                assert (exp != O.bbox_decode(b, dn)).any() or N < 3
            assert _same(got, exp), (entry, kw, N, C_)
            if raw is not None:
                assert _same(raw, dn)  # `raw` is the normed deltas bit for bit


@pytest.mark.parametrize("sigma", [0.3, 2.0])
def test_decode_tier2_vs_float64(O, dev, sigma):
    worst = 0.0
    for C_ in R.DECODE_C:
        for N in R.DECODE_N:
            rng = np.random.default_rng([N, C_, int(sigma * 10)])
            b, d = R.rois(rng, N), _deltas(rng, N, C_, sigma)
            for entry, kw in _decode_cases():
                kw = dict(kw, clamp=0)
                norm = (MEAN4, STD4) if kw.pop("norm", False) else None
                got, raw = run_decode(entry, b, d, N, C_, norm=norm, **kw)
                ref, bound = R.decode(b, d, *(norm or ())), R.decode_bound(b, d, *(norm or ()))
                ratio = float((np.abs(got.astype(F64) - ref) / bound).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (entry, kw, N, C_, ratio)
                if raw is not None:
                    assert _same(raw, O.bbox_norm(d, *norm) if norm else d)
    print("\nMEASURED decode sigma=%g: largest error / derived bound = %.3f" % (sigma, worst))


def test_decode_edge_boxes_and_deltas(O, dev):
    """zero-size and inverted boxes, coordinates of 1e30, dw = 88.8 (expf -> inf; inf * 0 -> NaN at w = 0), dw = -104, a NaN delta: inf / NaN by
    position as the fp32 rule gives them, the finite values within the derived bound of float64"""
    nan = np.nan
    boxes = np.array([[10, 20, 110, 220], [50, 60, 50, 60], [300, 40, 100, 20], [1e30, 1e30, 1e30, 1e30], [-1e30, 5, 1e30, 9], [1, 1, 1000, 600]], F32)
    dl = np.array([[0.1, -0.2, 0.3, 0.1], [0, 0, 88.8, 88.8], [0.5, 0.5, -104, -104], [nan, 0, 0, 0], [0, 0, nan, 0.2], [0, 0, 88.8, -104], [3, -3, 5, -5]], F32)
    C_ = dl.shape[0]
    N = boxes.shape[0]
    d = np.tile(dl.reshape(1, -1), (N, 1))
    with np.errstate(all="ignore"):
        emu, ref, bound = R.decode_f32(boxes, d), R.decode(boxes, d), R.decode_bound(boxes, d)
    assert np.isnan(emu[1].reshape(C_, 4)[1]).all()  # w = 0, dw = 88.8: inf * 0
    assert np.isinf(emu[0].reshape(C_, 4)[1]).all()
    e3 = emu[0].reshape(C_, 4)
    assert np.isnan(e3[3, [0, 2]]).all() and np.isfinite(e3[3, [1, 3]]).all() and np.isfinite(e3[2]).all()  # a NaN dx poisons x only, and only its own 4-vector
    for entry, kw in (("public", {}), ("fused", dict(clamp=0)), ("fused", dict(clamp=1)), ("head", dict(layout="5C+3", clamp=0)), ("head", dict(layout="5C", clamp=1))):
        got, _ = run_decode(entry, boxes, d, N, C_, **kw)
        exp = R.clamp(emu, 1000, 600) if kw.get("clamp") else emu
        fin = np.isfinite(exp)
        assert np.array_equal(np.isnan(got), np.isnan(exp)), (entry, kw)
        assert np.array_equal(got[np.isinf(exp)], exp[np.isinf(exp)])
        if kw.get("clamp"):
            cl = R.clamp(got, 1000, 600)
            assert _same(cl, got)  # already clamped; NaN passed through
            keep = fin & (exp == emu)  # values the clamp left alone
        else:
            keep = fin
        assert (np.abs(got.astype(F64) - ref)[keep] <= bound[keep]).all(), (entry, kw)
        assert np.array_equal(np.isnan(O.clamp_boxes(emu, 1000, 600)), np.isnan(emu))  # the oracle's clamp passes a NaN through too


def test_clamp_kernel(O, dev):
    up, dn = lambda v: np.nextafter(F32(v), F32(np.inf)), lambda v: np.nextafter(F32(v), F32(-np.inf))
    vals = [1, up(1), dn(1), 1000, up(1000), dn(1000), 600, up(600), dn(600), -0.0, 0.0, np.inf, -np.inf, np.nan, 3e38, -3e38, 300.5]
    v = np.array([(a, b) for a in vals for b in vals], F32)
    lib = _prod()
    for n_pairs in (1, 2, 255, 256, 257, v.shape[0]):
        x = v[:n_pairs] if n_pairs != 1 else v[13 * len(vals) + 3:][:1]

        def call():
            buf = _sent(2 * n_pairs + 6)
            buf[:2 * n_pairs] = _dev(x.reshape(-1))
            _ok(lib, lib.mpn_clamp_boxes(_p(buf), cs(n_pairs), cf(1000), cf(600), None))
            return (_np(buf),)
        got = twice(call)[0]
        assert _is_sent(got[2 * n_pairs:])
        exp = O.clamp_boxes(x, 1000, 600)
        assert _same(got[:2 * n_pairs].reshape(-1, 2), exp) and _same(exp, R.clamp(x, 1000, 600))
        assert np.array_equal(np.isnan(exp), np.isnan(x))  # the `<` / `>` chain passes a NaN through, in the oracle as in both kernels


# ---- augment merge ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C_", R.MERGE_MC)
def test_augment_merge_bit_equal(dev, M, C_):
    rng = np.random.default_rng([M, C_])
    W, H = 1000, 600
    lib = _dbg()
    big = F32(2 ** 24)
    for clamp in (0, 1):
        for regime in ("image", "edges", "big"):
            sA, sB = rng.random((M, C_), dtype=F32), rng.random((M, C_), dtype=F32)
            bA, bB = rng.uniform(-50, 1100, (M, 4 * C_)).astype(F32), rng.uniform(-50, 1100, (M, 4 * C_)).astype(F32)
            if regime == "edges":
                pick = np.array([1, W, W + 1, np.nextafter(F32(1), F32(0)), np.nextafter(F32(W), F32(2 * W))], F32)
                bA, bB = rng.choice(pick, bA.shape).astype(F32), rng.choice(pick, bB.shape).astype(F32)
                sA.flat[0], sB.flat[0] = 3e38, 3e38  # the sum overflows: inf * 0.5
            elif regime == "big":  # (-x + W) + 1 rounds twice near 2^24
                bB = (big - rng.integers(0, 4000, bB.shape)).astype(F32)
                bA = (big - rng.integers(0, 4000, bA.shape)).astype(F32) * rng.choice(np.array([1, -1], F32), bA.shape)
            with np.errstate(over="ignore"):
                es, eb = A.merge(sA, bA, sB, bB, W, H, clamp=bool(clamp))

            def call():
                s_io, b_io = _sent(M * C_ + 3), _sent(4 * M * C_ + 5)
                s_io[:M * C_], b_io[:4 * M * C_] = _dev(sB.reshape(-1)), _dev(bB.reshape(-1))
                sAd, bAd = _dev(sA), _dev(bA)
                _ok(lib, lib.mpn_debug_head_post(MERGE, _p(sAd), _p(bAd), 0, 0, M, C_, 0, None, None, clamp, float(W), float(H), _p(s_io), _p(b_io), None))
                return _np(s_io), _np(b_io)
            gs, gb = twice(call)
            assert _is_sent(gs[M * C_:]) and _is_sent(gb[4 * M * C_:])
            assert _same(gs[:M * C_], es.reshape(-1)) and _same(gb[:4 * M * C_], eb.reshape(-1)), (regime, clamp)
            if regime == "edges":
                assert np.isinf(gs[0])


# ---- per-class selection ---------------------------------------------------------------------------------------------------------------
def _select_inputs(rng, N, C_, regime):
    s = (np.round(rng.random((N, C_)) * 64) / 64).astype(F32)
    if regime == "equal":
        s[7::256] = F32(0.5)  # the threshold itself, once in every block of 256 rows, in every class
        s[N - 1] = F32(0.5)
    elif regime == "zeros":
        s = np.where(rng.random((N, C_)) < 0.5, F32(-0.0), F32(0.0)).astype(F32)
        s[rng.random((N, C_)) < 0.2] = F32(0.25)
    elif regime == "nan":
        s[rng.random((N, C_)) < 0.3] = np.nan
    bbox = rng.uniform(1, 600, (N, 4 * C_)).astype(F32)
    return s, bbox


@pytest.mark.parametrize("C_", R.SELECT_C)
def test_select_scored_bit_equal(O, dev, C_):
    lib = _prod()
    for N in R.SELECT_N:
        for fi, first_cls in enumerate(sorted({0, 1, C_ - 1, C_})):
            for ri, (regime, thresh) in enumerate((("equal", 0.5), ("equal", -1.5), ("equal", 2.0), ("zeros", 0.0), ("nan", 0.25))):
                rng = np.random.default_rng([N, C_, first_cls, ri])
                s, bbox = _select_inputs(rng, N, C_, regime)
                n_cls = C_ - first_cls
                with_idx = (fi + ri) % 2 == 0  # a NULL d_src_idx in every other case

                def call():
                    scored = _sent(n_cls + 1, N, 5)  # one slab more than the classes: it must keep the sentinel
                    counts = torch.full((n_cls + 1,), -7, dtype=torch.int32, device=scored.device)
                    src = torch.full((n_cls + 1, N), -7, dtype=torch.int32, device=scored.device) if with_idx else None
                    sd, bd = _dev(s), _dev(bbox)
                    _ok(lib, lib.mpn_select_scored(_p(sd), _p(bd), N, C_, first_cls, cf(thresh), _p(scored), _p(counts), _p(src), None))
                    return (_np(scored), _np(counts)) + ((_np(src),) if with_idx else ())
                res = twice(call)
                scored, counts = res[0], res[1]
                assert _is_sent(scored[n_cls:]) and (counts[n_cls:] == -7).all() and (not with_idx or (res[2][n_cls:] == -7).all())
                if n_cls == 0:
                    continue
                for j in range(n_cls):
                    sb, idx = O.select_scored(s, bbox, first_cls + j, thresh)
                    n = int(counts[j])
                    assert n == sb.shape[0], (N, C_, first_cls, regime, thresh, j)
                    assert _same(scored[j, :n], sb) and _is_sent(scored[j, n:])
                    if with_idx:
                        assert np.array_equal(res[2][j, :n], idx) and (res[2][j, n:] == -7).all()
                    if regime == "nan":
                        assert not np.isnan(sb[:, 4]).any()  # s > thresh drops a NaN score
                    if thresh == 2.0:
                        assert n == 0
                    if thresh == -1.5:
                        assert n == N


def test_select_boxes_bit_equal(O, dev):
    lib = _prod()
    for N in R.SELECT_N:
        for C_ in R.SELECT_C:
            rng = np.random.default_rng([N, C_, 5])
            s, bbox = _select_inputs(rng, N, C_, "nan")  # quantised scores: ties everywhere (the first maximum wins); NaNs: never picked past column 0
            s[::5, 0] = np.nan

            def call():
                out = _sent(N + 2, 4)
                sd, bd = _dev(s), _dev(bbox)
                _ok(lib, lib.mpn_select_boxes_forward(_p(sd), _p(bd), N, C_, _p(out), None))
                return (_np(out),)
            got = twice(call)[0]
            assert _is_sent(got[N:]) and _same(got[:N], O.select_boxes(s, bbox))
            assert _same(got[:N:5], bbox[::5, :4])  # v > NaN is never true: a NaN in column 0 keeps class 0


# ---- bbox_vote -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _vote_case(m):
    from oracle import mpn_oracle as O
    sb = R.vote_tables(np.random.default_rng(m), m)
    return sb, O.nms(sb, 0.7)  # keeps are NMS survivors of the table itself: every kept box overlaps itself


def run_vote(nb, sb, n_arg, thr, d_n=None, pad_rows=2):
    lib = _prod()

    def call():
        res = _sent(n_arg + pad_rows, 5)
        # 256 rows past m that must not be read: copies of kept box 0 with a weight that would outvote everything
        poison = np.tile(np.concatenate([nb[0, :4], [1e6]]).astype(F32), (256, 1))
        nd, sd = _dev(nb), _dev(np.concatenate([sb, poison]))
        dn = torch.tensor([d_n], dtype=torch.int32, device=res.device) if d_n is not None else None
        _ok(lib, lib.mpn_bbox_vote(_p(nd), n_arg, _p(dn), _p(sd), sb.shape[0], cf(thr), _p(res), None))
        return (_np(res),)
    return twice(call)[0]


@pytest.mark.parametrize("m", R.VOTE_M)
def test_bbox_vote_bit_equal_and_vs_float64(O, dev, m):
    sb, keep = _vote_case(m)
    worst = 0.0
    for n in R.VOTE_N_NMS:
        nb = keep[:n]
        n = nb.shape[0]
        got = run_vote(nb, sb, n, 0.3)
        assert _is_sent(got[n:])
        exp = O.bbox_vote(nb, sb, 0.3)
        assert _same(got[:n], exp), (m, n)
        if O.have_ref():
            assert _same(got[:n], O.ref_bbox_vote(nb, sb, 0.3))
        ref, bound = R.vote(nb, sb, 0.3)
        ratio = float((np.abs(got[:n, :4] - ref[:, :4]) / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0 and np.array_equal(got[:n, 4], nb[:, 4])
        if n > 1:  # *d_n_nms below n_nms: the rows from it on keep the sentinel
            part = run_vote(nb, sb, n, 0.3, d_n=n // 2)
            assert _same(part[:n // 2], exp[:n // 2]) and _is_sent(part[n // 2:])
    # a kept box whose voters all have score 0: 0 / 0
    z = sb.copy()
    z[:, 4] = 0
    got = run_vote(keep[:3], z, min(3, keep.shape[0]), 0.3)[:min(3, keep.shape[0])]
    assert np.isnan(got[:, :4]).all() and _same_nanpos(got, O.bbox_vote(keep[:3], z, 0.3))
    print("\nMEASURED bbox_vote m=%d: largest error / derived bound = %.3f" % (m, worst))


@pytest.mark.parametrize("score_pow", R.VOTE_POW)
@pytest.mark.parametrize("n_cls", [1, 7, 20])
def test_bbox_vote_batched(O, dev, n_cls, score_pow):
    lib = _prod()
    stride = 333  # not a multiple of the 256-row tile
    rng = np.random.default_rng([n_cls, int(score_pow * 10)])
    counts = rng.integers(1, stride + 1, n_cls)
    counts[0] = stride  # a full class
    tables, keeps = [], []
    for c in range(n_cls):
        sb = R.vote_tables(rng, int(counts[c]))
        if c == 2:
            sb[:, 4] = 0  # every weight 0: 0 / 0
        if c == 3:
            sb[::4, 4] *= -1  # negative scores: NaN weights under pow 0.5
        tables.append(sb)
        keeps.append(O.nms(np.abs(sb), 0.7))
    n_keep = np.array([k.shape[0] if c % 2 else min(k.shape[0], 65) for c, k in enumerate(keeps)])
    if n_cls > 1:
        counts[1], n_keep[1] = 0, 0  # an empty class
    if n_cls > 5:
        counts[5] = 0  # kept boxes without a voter: 0 / 0
    for use_counts in (True, False):
        keep_t, scored_t = np.full((n_cls, stride, 5), 7.0, F32), np.full((n_cls, stride, 5), 7.0, F32)
        for c in range(n_cls):
            keep_t[c, :keeps[c].shape[0]] = keeps[c]
            scored_t[c, :tables[c].shape[0]] = tables[c]
            if keeps[c].shape[0]:  # the rows past counts[c] would outvote everything for kept box 0 if a tile read them
                scored_t[c, tables[c].shape[0]:] = np.concatenate([keeps[c][0, :4], [1e6]]).astype(F32)
        if not use_counts:  # counts == NULL: every class votes over all m_stride rows
            scored_t[:, :, :] = np.stack([R.vote_tables(np.random.default_rng([c, 9]), stride) for c in range(n_cls)])

        def call():
            res = _sent(n_cls, stride, 5)
            kd, sd = _dev(keep_t), _dev(np.concatenate([scored_t, np.full((1, stride, 5), 1e6, F32)]))  # a slab past the last class: not to be read
            nk, cn = _dev(n_keep, np.int32), (_dev(counts, np.int32) if use_counts else None)
            _ok(lib, lib.mpn_bbox_vote_batched(_p(kd), _p(nk), _p(sd), _p(cn), n_cls, stride, cf(0.3), cf(score_pow), _p(res), None))
            return (_np(res),)
        got = twice(call)[0]
        for c in range(n_cls):
            nk = int(n_keep[c])
            assert _is_sent(got[c, nk:]), (c, "wrote rows past n_keep")
            if nk == 0:
                continue
            sb = scored_t[c, :int(counts[c])] if use_counts else scored_t[c]
            exp = R.vote_f32(keep_t[c, :nk], sb, 0.3, score_pow)
            assert _same_nanpos(got[c, :nk], exp), (n_cls, score_pow, use_counts, c)
            if score_pow == 1.0:
                assert _same_nanpos(got[c, :nk], O.bbox_vote(keep_t[c, :nk], sb, 0.3))
            ref, bound = R.vote(keep_t[c, :nk], sb, 0.3, score_pow)
            ok = np.isfinite(ref[:, :4]) & np.isfinite(bound)
            assert (np.abs(got[c, :nk, :4] - ref[:, :4])[ok] <= bound[ok]).all()
            if use_counts and c in (2, 5):
                assert np.isnan(got[c, :nk, :4]).all()


# ---- image.scale -----------------------------------------------------------------------------------------------------------------------
def run_scale(im, H2, W2):
    lib = _prod()
    Cc, H, W = im.shape

    def call():
        out = _sent(Cc * H2 * W2 + 5)
        tmp = _sent(Cc * H * W2 + 5)
        xd = _dev(im)
        _ok(lib, lib.mpn_image_scale(_p(xd), Cc, H, W, H2, W2, _p(tmp), _p(out), None))
        return _np(out), _np(tmp)
    out, tmp = twice(call)
    assert _is_sent(out[Cc * H2 * W2:]) and _is_sent(tmp[Cc * H * W2:])
    return out[:Cc * H2 * W2].reshape(Cc, H2, W2)


@pytest.mark.parametrize("H,W,H2,W2,Cc", R.scale_cases())
def test_image_scale_bit_equal_and_vs_float64(O, dev, H, W, H2, W2, Cc):
    im = np.random.default_rng(H * 1009 + W).random((Cc, H, W), dtype=F32)
    got = run_scale(im, H2, W2)
    assert _same(got, O.image_scale(im, H2, W2))
    assert (np.abs(got - R.image_scale(im, H2, W2)) <= R.image_scale_bound(H, W, H2, W2, 1.0)).all()
    for v in (1.0, 0.5, -2.0):  # a power-of-two constant comes back bit for bit (tests/test_boxes_ref_cpu.py says why only those)
        assert _same(run_scale(np.full((Cc, H, W), F32(v)), H2, W2), np.full((Cc, H2, W2), F32(v)))


# ---- small companions ------------------------------------------------------------------------------------------------------------------
def _edge_boxes(rng, n):
    b = R.rois(rng, n) if n else np.zeros((0, 4), F32)
    if n >= 4:
        b[1, 2:] = b[1, :2]  # zero size
        b[2] = b[2, [2, 3, 0, 1]]  # inverted
        b[3] = F32(1e30)
    if n >= 6:
        b[5] = [-1e30, 5, 1e30, 9]
    return b


@pytest.mark.parametrize("n", R.COMPANION_N)
def test_small_companions_bit_equal(O, dev, n):
    lib = _prod()
    rng = np.random.default_rng(n + 11)
    b = _edge_boxes(rng, n)
    rois = np.concatenate([np.ones((n, 1), F32), b], 1)
    dets = np.concatenate([b, rng.random((n, 1), dtype=F32), rng.integers(1, 5, (n, 1)).astype(F32)], 1)
    cats = np.array([3, 17, 44, 90], F32)

    def run(shape, fn, init=None):
        def call():
            out = _sent(*shape)
            if init is not None:
                out.view(-1)[:init.size] = _dev(init.reshape(-1))
            fn(out)
            return (_np(out),)
        return twice(call)[0]

    rd, bd, dd, cd = _dev(rois.reshape(-1, 5)), _dev(b.reshape(-1, 4)), _dev(dets.reshape(-1, 6)), _dev(cats)
    with np.errstate(all="ignore"):
        got = run((4 * n + 1, 5), lambda o: _ok(lib, lib.mpn_foveal_forward(_p(rd), n, _p(o), None)))
        assert _is_sent(got[4 * n:]) and _same_nanpos(got[:4 * n], O.foveal(rois))
        for scale in (1.5, 0.5):
            got = run((n + 1, 5), lambda o: _ok(lib, lib.mpn_context_region_forward(_p(rd), n, C.c_double(scale), _p(o), None)))
            assert _is_sent(got[n:]) and _same_nanpos(got[:n], O.context_region(rois, scale))
        m4, s4 = (C.c_float * 4)(*MEAN4), (C.c_float * 4)(*STD4)
        d = np.tile(b, (1, 3))
        got = run((n + 1, 12), lambda o: _ok(lib, lib.mpn_bbox_norm_forward(_p(o), n, 12, m4, s4, None)), init=d)
        assert _is_sent(got[n:]) and _same_nanpos(got[:n], O.bbox_norm(d, MEAN4, STD4) if n else d)
        for s in (1.0, 0.731):
            got = run((n + 1, 5), lambda o: _ok(lib, lib.mpn_project_im_rois(_p(bd), n, C.c_double(s), _p(o), None)))
            assert _is_sent(got[n:]) and _same_nanpos(got[:n], O.project_im_rois(b, s))
        got = run((n + 1, 7), lambda o: _ok(lib, lib.mpn_dets_to_coco_rows(_p(dd), None, n, cf(42), _p(cd), 4, _p(o), None)))
        assert _is_sent(got[n:]) and _same_nanpos(got[:n], O.coco_rows(dets, 42, cats) if n else np.zeros((0, 7), F32))
        if n > 2:  # *d_n_dets below max_n: the rows from it on keep the sentinel
            nd = torch.tensor([n - 2], dtype=torch.int32, device=dd.device)
            got = run((n + 1, 7), lambda o: _ok(lib, lib.mpn_dets_to_coco_rows(_p(dd), _p(nd), n, cf(42), _p(cd), 4, _p(o), None)))
            assert _is_sent(got[n - 2:]) and _same_nanpos(got[:n - 2], O.coco_rows(dets[:n - 2], 42, cats))
        yx = b[:, [1, 0, 3, 2]].copy()
        yd = _dev(yx.reshape(-1, 4))
        for area in (0.0, 2000.0):
            keep = torch.full((n + 1,), -7, dtype=torch.int32, device=yd.device)
            got = run((n + 1, 4), lambda o: _ok(lib, lib.mpn_proposals_permute_filter(_p(yd), n, cf(area), _p(o), _p(keep), None)))
            assert _is_sent(got[n:]) and _same(got[:n], b)
            kept = _np(keep)
            assert kept[n] == -7
            exp_b, _ = O.prepare_proposals(yx, None, area)
            assert _same(b[kept[:n] == 1], exp_b)


# ---- the pointer contract --------------------------------------------------------------------------------------------------------------
def test_misaligned_pointers_are_refused_before_launch(dev):
    """include/mpn.h: mpn_bbox_decode (16 bytes, all three), mpn_clamp_boxes (8), mpn_select_scored (d_bbox, 16).  Asked for the refusal only: the
    answer comes before anything is launched, so the output keeps its sentinel."""
    lib = _prod()
    buf, out = _dev(np.zeros(4096, F32)), _sent(4096)
    base, o = buf.data_ptr(), out.data_ptr()
    assert base % 16 == 0 and o % 16 == 0
    vp = C.c_void_p
    for off, arg in ((4, "d_boxes"), (8, "d_boxes")):
        assert lib.mpn_bbox_decode(vp(base + off), vp(base), 4, 2, vp(o), None) == MPN_EINVAL and arg in _err(lib) and "16-byte" in _err(lib)
    assert lib.mpn_bbox_decode(vp(base), vp(base + 4), 4, 2, vp(o), None) == MPN_EINVAL and "d_deltas" in _err(lib)
    assert lib.mpn_bbox_decode(vp(base), vp(base), 4, 2, vp(o + 12), None) == MPN_EINVAL and "d_out" in _err(lib)
    assert lib.mpn_bbox_decode(vp(base + 4), vp(base), 0, 2, vp(o), None) == MPN_EINVAL  # N = 0 does not excuse it
    assert lib.mpn_clamp_boxes(vp(o + 4), cs(8), cf(10), cf(10), None) == MPN_EINVAL and "d_bbox" in _err(lib) and "8-byte" in _err(lib)
    cnt = torch.zeros(4, dtype=torch.int32, device=buf.device)
    assert lib.mpn_select_scored(vp(base), vp(base + 8), 4, 2, 0, cf(0.5), vp(o), _p(cnt), None, None) == MPN_EINVAL and "d_bbox" in _err(lib)
    assert lib.mpn_select_scored(vp(base + 4), vp(base + 16), 4, 2, 0, cf(0.5), vp(o), _p(cnt), None, None) == 0  # d_scores needs 4 bytes only
    assert lib.mpn_clamp_boxes(vp(o + 8), cs(0), cf(10), cf(10), None) == 0
    dl = _dbg()
    assert dl.mpn_debug_bbox_decode_clamp(base + 4, base, 4, 2, o, 1, 10.0, 10.0, None) == MPN_EINVAL
    torch.cuda.synchronize()
    assert _is_sent(out.cpu().numpy()[64:])


def test_utils_decode_copies_a_misaligned_view(O, dev):
    """the in-tree callers of mpn_bbox_decode pass fresh allocations or rows of a table; a contiguous view that starts inside a row is copied"""
    from multipathnet_amd import utils
    rng = np.random.default_rng(3)
    b, d = R.rois(rng, 9), _deltas(rng, 9, 2, 0.3, tier1=True)
    flat_b, flat_d = _dev(np.concatenate([[0], b.reshape(-1)])), _dev(np.concatenate([[0], d.reshape(-1)]))
    vb, vd = flat_b[1:].view(9, 4), flat_d[1:].view(9, 8)
    assert vb.data_ptr() % 16 == 4 and vb.is_contiguous()
    assert _same(_np(utils.decode_all_classes(vb, vd)), O.bbox_decode(b, d))
    # two column views (utils.lua narrows both): each needs a copy, and the two copies must not share a block (see the module docstring)
    wide_b, wide_d = _dev(np.concatenate([np.zeros((9, 1), F32), b], 1)), _dev(np.concatenate([d[:, 4:], d[:, :4]], 1))
    out = torch.empty((9, 4), dtype=torch.float32, device=wide_b.device)
    utils.convertFrom(out, wide_b[:, 1:], wide_d[:, 4:])
    assert _same(_np(out), O.bbox_decode(b, d[:, :4].copy()))
