"""Every launch form of the linear-GEMM family (dense.hip: gemm_c8_pf_kernel and its split-K / row-invariant / residual / per-row-scaled
forms, and the three-plane bf16 split of MPN_FC_SPLIT3) against a float64 product computed on the host.

Forms are reached one at a time through mpn_debug_linear_form (debug flavour only); the product dispatch through mpn_linear_forward on the
library that ships.  Four kinds of check:
  * exact: operands whose every partial sum is representable (small integers; sparse rows of 20-bit values against +-2^e weights), so any
    summation order gives the float64 value bit for bit and a dropped, repeated or misplaced K chunk or row changes the result;
  * accuracy on four data sets, e = |y - y64| / (sum_k |x_k w_k| + |b|) against the error of the oracle's sequential fp32 chain (O.linear);
  * edge operands: |x| near FLT_MAX, +-inf / NaN (every output in the float64 result's class: NaN, +inf, -inf or finite), subnormals;
  * the plane split itself, row invariance, and the per-row scales of the pad rows of the MultiPathNet mix GEMM.
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import hooks

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # fp32 unit roundoff
BF16_OVERFLOW = float(np.float32(np.uint32(0x7F7F8000).view(np.float32)))  # 0x1.fep127 = 3.3962e38: RNE to bf16 gives inf from here up
FLT_MAX = float(np.finfo(np.float32).max)
KNOB_DEFAULTS = dict(gemm_kch=0, gemm_split=0, gemm_rsi=1, split3_ranges=0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the forms
# ---------------------------------------------------------------------------------------------------------------------------------------
def _form_table():
    f = {
        "product": dict(form=None),
        "kch4": dict(form=0, knobs=dict(gemm_kch=4)),
        "kch8": dict(form=0, knobs=dict(gemm_kch=8)),
        "split2": dict(form=0, knobs=dict(gemm_split=2)),
        "split5": dict(form=0, knobs=dict(gemm_split=5)),
        "kch8_split2": dict(form=0, knobs=dict(gemm_kch=8, gemm_split=2)),
        "ri1": dict(form=0, ri=1),
        "ri2": dict(form=0, ri=2),
        "ri2_res": dict(form=0, ri=2, res=True),
        "res": dict(form=0, res=True),  # the direct form: >= 128 output tiles only
    }
    for n in (1, 2, 3):
        for mode, rsi in (("rsi", 1), ("fold", 0)):
            for packed in (0, 1):
                f["rs%d_%s%s" % (n, mode, "_packed" if packed else "")] = dict(form=1, n_seg=n, packed=packed, knobs=dict(gemm_rsi=rsi))
    for r in (0, 1, 3, 8):
        f["split3_%s" % (r or "auto")] = dict(form=2, knobs=dict(split3_ranges=r))
    return f


FORMS = _form_table()

# straddle every padding boundary: rows (tiles of 128, packed bins of 4 / 8), K (chunks of 8, stages of 32 / 64, split3 k16 steps and
# ranges), N (tiles of 128, split3's 256-row weight tiles); fc6 (K = 25088, N = 4096) at 1000 and 37 rows
SHAPES = [(1, 1, 1), (7, 7, 3), (8, 8, 127), (127, 31, 129), (128, 33, 255), (129, 63, 257), (255, 64, 1), (257, 65, 3),
          (1000, 300, 127), (1001, 4096, 129), (1, 25088, 4097), (37, 25088, 4096), (1000, 25088, 4096), (7, 25089, 3), (129, 65, 4097),
          (255, 300, 257), (257, 4096, 255), (1001, 33, 1), (128, 64, 129), (127, 7, 257), (8, 1, 255), (1000, 63, 3), (129, 4096, 127),
          (257, 31, 4097), (1001, 300, 4097), (255, 25089, 129), (1, 300, 257), (128, 8, 4097), (7, 64, 129), (1000, 1, 1)]


def _tiles(M, N):
    return ((M + 127) // 128) * ((N + 127) // 128)


def _cuts(K):
    """K-segment ends (multiples of 32 below K): the 3-segment cuts (c1, c2); the 2-segment form cuts at c2 alone"""
    c = list(range(32, K, 32))
    if not c:
        return None, None
    if len(c) == 1:
        return None, c[0]
    c1, c2 = c[len(c) // 3], c[(2 * len(c)) // 3]
    return (c1, c2) if c2 != c1 else (c1, c[-1])


def _applies(form, M, K, N):
    f = FORMS[form]
    if form == "res":
        return _tiles(M, N) >= 128
    if f["form"] == 1:
        c1, c2 = _cuts(K)
        if f["n_seg"] == 3 and c1 is None or f["n_seg"] == 2 and c2 is None:
            return False
        if f["packed"] and M % 4:
            return False
    return True


def _bin_rows(M):
    return 8 if M % 8 == 0 else 4


@functools.lru_cache(maxsize=None)
def _dbg():
    from multipathnet_amd import _lib
    lib = _lib.load("debug")
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    lib.mpn_debug_linear_form.argtypes = [vp, i, i, vp, vp, i, i, i, i, vp, i, C.POINTER(C.c_int), vp, i, i, i, vp, vp, sz]
    lib.mpn_debug_split3_planes.argtypes = [vp, i, vp]
    lib.mpn_debug_l2norm_row_scales.argtypes = [vp, i, i, i, vp, i, i, i, i, C.c_float, i, C.c_float, vp]
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


def run_form(form, x, w, b, relu=0, scales=None, cuts=(), raw=False):
    """y[M, N] (numpy float32) of one form; scales [n_seg, rs_mod] for the row-scaled forms.  raw=True also returns the C8 output buffer as
    [pitch, NP] (rows x channels) and the packed form's (bins, bin_rows, out_Mp)."""
    from multipathnet_amd import _lib
    f = FORMS[form]
    M, K = x.shape
    N = w.shape[0]
    dev = torch.device("cuda", 0)
    xd, wd = torch.from_numpy(np.ascontiguousarray(x)).to(dev), torch.from_numpy(np.ascontiguousarray(w)).to(dev)
    bd = torch.from_numpy(np.ascontiguousarray(b)).to(dev) if b is not None else None
    if f["form"] is None:  # the product dispatch on the product library
        lib = _lib.load("product")
        y = torch.empty((M, N), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        _lib.check(lib.mpn_linear_forward(_ptr(xd), M, K, _ptr(wd), _ptr(bd), N, int(relu), _ptr(y), None), "mpn_linear_forward")
        torch.cuda.synchronize()
        return y.cpu().numpy()
    lib = _dbg()
    res = None
    if f.get("res"):
        res = torch.from_numpy(_residual(M, N)).to(dev)
    n_seg, rs_mod, bin_rows, out_Mp, kend = 0, 0, 0, 0, None
    sd = None
    if f["form"] == 1:
        n_seg = f["n_seg"]
        rs_mod = scales.shape[1]
        sd = torch.from_numpy(np.ascontiguousarray(scales[:n_seg], dtype=np.float32)).to(dev)
        kend = (C.c_int * 2)(*(list(cuts) + [0, 0])[:2])
        if f["packed"]:
            bin_rows = _bin_rows(M)
            out_Mp = bin_rows + 8  # a gap of never-written rows between bins: the scatter must leave it alone
    pitch = (M // bin_rows) * out_Mp if bin_rows else (M + 127) // 128 * 128
    NP = (N + 127) // 128 * 128
    y = torch.empty((pitch if bin_rows else M, N), dtype=torch.float32, device=dev)
    rawd = torch.empty(NP * pitch, dtype=torch.float32, device=dev) if raw else None
    torch.cuda.synchronize()
    with _knobs(lib, **f.get("knobs", {})):
        rc = lib.mpn_debug_linear_form(_ptr(xd), M, K, _ptr(wd), _ptr(bd), N, int(relu), f["form"], f.get("ri", 0), _ptr(res), n_seg, kend,
                                       _ptr(sd), rs_mod, bin_rows, out_Mp, _ptr(y), _ptr(rawd), NP * pitch if raw else 0)
    if rc != 0:
        raise _lib.MpnError("mpn_debug_linear_form(%s) failed (%d): %s" % (form, rc, lib.mpn_last_error().decode()))
    yh = y.cpu().numpy()
    if bin_rows:  # (bin, roi) rows back in order
        yh = yh.reshape(M // bin_rows, out_Mp, N)[:, :bin_rows].reshape(M, N)
    if not raw:
        return yh
    r = rawd.cpu().numpy().reshape(NP // 8, pitch, 8).transpose(1, 0, 2).reshape(pitch, NP)
    return yh, r, (M // bin_rows if bin_rows else 0, bin_rows, out_Mp)


def _residual(M, N):
    return (np.arange(M * N, dtype=np.int64).reshape(M, N) % 7 - 3).astype(np.float32)


def _seg_bounds(form, K, cuts3):
    """segment column ranges of a row-scaled form and the host cut list it is given"""
    n = FORMS[form]["n_seg"]
    c1, c2 = cuts3
    if n == 1:
        return [(0, K)], []
    if n == 2:
        return [(0, c2), (c2, K)], [c2]
    return [(0, c1), (c1, c2), (c2, K)], [c1, c2]


def _parts(x, w, cuts3):
    """float64 products of the K ranges [0, c1), [c1, c2), [c2, K) (an absent cut: an empty range) — every form's reference is a
    combination of these three, so a shape's big product is computed once"""
    K = x.shape[1]
    c1, c2 = cuts3
    c2 = c2 or 0
    c1 = c1 or c2
    out = []
    for k0, k1 in ((0, c1), (c1, c2), (c2, K)):
        out.append(x[:, k0:k1].astype(np.float64) @ w[:, k0:k1].astype(np.float64).T if k1 > k0 else 0.0)
    return out


def ref64(form, x, w, b, relu, scales=None, cuts3=(None, None), parts=None):
    """float64 y of a form on finite data (BLAS; per-K-segment scales for the row-scaled forms)"""
    f = FORMS[form]
    M = x.shape[0]
    pa, pb, pc = parts if parts is not None else _parts(x, w, cuts3)
    if f["form"] == 1:
        rows = np.arange(M) % scales.shape[1]
        s = [scales[i, rows].astype(np.float64)[:, None] for i in range(3)]
        n = f["n_seg"]
        if n == 1:
            y = s[0] * (pa + pb + pc)
        elif n == 2:
            y = s[0] * (pa + pb) + s[1] * pc
        else:
            y = s[0] * pa + s[1] * pb + s[2] * pc
        y = y + np.zeros((M, w.shape[0]))
    else:
        y = pa + pb + pc + np.zeros((M, w.shape[0]))
    if b is not None:
        y = y + b.astype(np.float64)
    if f.get("res"):
        y = y + _residual(*y.shape)
    return np.where(y < 0, 0.0, y) if relu else y


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. exact tests
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _dense_case(M, K, N):
    """small integers, |x|, |w|, |b| <= 3: sum |x w| <= 9 K + 3 < 2^18 for every K here, so every partial sum — with row scales of 1/2, 1
    or 2 and the in-place form's ratios of them (1/4 .. 4) — is a multiple of 1/4 below 2^22: exact in fp32 in any order"""
    rng = np.random.default_rng(M * 1000003 + K * 1009 + N)
    x = rng.integers(-3, 4, (M, K)).astype(np.float32)
    w = rng.integers(-3, 4, (N, K)).astype(np.float32)
    b = rng.integers(-3, 4, N).astype(np.float32)
    scales = (2.0 ** rng.integers(-1, 2, (3, M))).astype(np.float32)  # rs_mod = M: one scale per row and segment
    return x, w, b, scales, _parts(x, w, _cuts(K))


EXACT_CASES = [(s, f) for s in SHAPES for f in FORMS if _applies(f, *s)]


@pytest.mark.parametrize("shape,form", EXACT_CASES, ids=["%dx%dx%d-%s" % (s + (f,)) for s, f in EXACT_CASES])
def test_exact_small_integers(dev, shape, form):
    M, K, N = shape
    x, w, b, scales, parts = _dense_case(M, K, N)
    relu = (M + K + N) % 2
    cuts3 = _cuts(K)
    _, cuts = _seg_bounds(form, K, cuts3) if FORMS[form]["form"] == 1 else (None, [])
    y = run_form(form, x, w, b, relu=relu, scales=scales, cuts=cuts)
    y64 = ref64(form, x, w, b, relu, scales, cuts3, parts)
    bad = np.argwhere(y.astype(np.float64) != y64)
    assert bad.size == 0, "%d of %d outputs differ, first at (row, col) %s: %r vs %r" % (
        len(bad), y.size, tuple(bad[0]), float(y[tuple(bad[0])]), float(y64[tuple(bad[0])]))


@functools.lru_cache(maxsize=1)
def _sparse_case(M, K, N, seed):
    """<= 8 non-zeros per row at random K positions (one of them in the last partial chunk when there is one), each a multiple of 2^-16
    below 2^4 (20 significant bits: all three bf16 planes), against weights +-2^e (e fixed per output column, so the <= 8 products of a
    sum share one grid: < 2^(e + 7) on a 2^(e - 16) grid — exact in fp32)"""
    rng = np.random.default_rng(seed)
    x = np.zeros((M, K), np.float32)
    nz = min(8, K)
    tail0 = (K - 1) // 8 * 8
    for m in range(M):
        cols = rng.choice(K, nz, replace=False)
        cols[0] = rng.integers(tail0, K)  # the last (possibly partial) chunk
        x[m, cols] = (rng.integers(-(2 ** 20) + 1, 2 ** 20, nz) * 2.0 ** -16).astype(np.float32)
    e = rng.integers(-3, 4, N)
    w = (rng.choice([-1.0, 1.0], (N, K)) * (2.0 ** e)[:, None]).astype(np.float32)
    return x, w, _parts(x, w, _cuts(K))


SPARSE_SHAPES = [(7, 7, 3), (127, 31, 129), (129, 63, 257), (257, 65, 3), (1000, 300, 127), (129, 4096, 127), (37, 25088, 4096),
                 (7, 25089, 3), (255, 25089, 129), (128, 33, 255)]
SPARSE_CASES = [(s, f) for s in SPARSE_SHAPES for f in FORMS if _applies(f, *s)]


@pytest.mark.parametrize("shape,form", SPARSE_CASES, ids=["%dx%dx%d-%s" % (s + (f,)) for s, f in SPARSE_CASES])
def test_exact_sparse_three_plane_values(dev, shape, form):
    """(row scales all 1: the in-place form's ratios then stay exact on these 23-bit sums)"""
    M, K, N = shape
    x, w, parts = _sparse_case(M, K, N, seed=M + 7 * K + 13 * N)
    scales = np.ones((3, M), np.float32)
    cuts3 = _cuts(K)
    _, cuts = _seg_bounds(form, K, cuts3) if FORMS[form]["form"] == 1 else (None, [])
    y = run_form(form, x, w, None, scales=scales, cuts=cuts)
    y64 = ref64(form, x, w, None, 0, scales, cuts3, parts)
    bad = np.argwhere(y.astype(np.float64) != y64)
    assert bad.size == 0, "%d outputs differ, first at %s: %r vs %r" % (len(bad), tuple(bad[0]), float(y[tuple(bad[0])]),
                                                                        float(y64[tuple(bad[0])]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. accuracy against float64, beside the oracle's sequential fp32 chain
# ---------------------------------------------------------------------------------------------------------------------------------------
def _acc_data(kind, M, K, N, seed):
    rng = np.random.default_rng(seed)
    b = rng.standard_normal(N).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    if kind == "normal":
        x = rng.standard_normal((M, K))
    elif kind == "positive":  # ReLU outputs against positive weights: every partial sum grows, the chain's error fastest
        x = np.abs(rng.standard_normal((M, K)))
        w = np.abs(w)
    elif kind == "cancel":  # rows of +-pairs against equal weight pairs: sum |x w| large, y small
        h = rng.standard_normal((M, (K + 1) // 2))
        x = np.stack([h, -h * (1 + 2.0 ** -10 * rng.standard_normal(h.shape))], 2).reshape(M, -1)[:, :K]
        w[:, 1::2] = w[:, 0:K - K % 2:2][:, :w[:, 1::2].shape[1]]
    elif kind == "wide":  # per-k magnitudes 2^-40 .. 2^40
        x = rng.choice([-1.0, 1.0], (M, K)) * 2.0 ** rng.uniform(-40, 40, (M, K))
    return np.ascontiguousarray(x, dtype=np.float32), w, b


def _err(y, y64, D):
    e = np.abs(y.astype(np.float64) - y64) / D
    return float(e.max()), float(np.sqrt((e * e).mean()))


ACC_SHAPES = [(129, 1024, 257), (256, 4096, 129)]
ACC_FORMS = ["product", "kch8", "split2", "split5", "ri1", "ri2", "rs3_rsi", "rs3_fold", "rs2_rsi_packed", "split3_auto", "split3_1"]
ACC_KINDS = ["normal", "positive", "cancel", "wide"]
ACC_CASES = [(s, k, f) for s in ACC_SHAPES for k in ACC_KINDS for f in ACC_FORMS if _applies(f, *s)]


@functools.lru_cache(maxsize=1)
def _acc_case(kind, M, K, N):
    x, w, b = _acc_data(kind, M, K, N, seed=ACC_KINDS.index(kind) * 7919 + M * 31 + K)
    rng = np.random.default_rng(K + M)
    scales = rng.uniform(0.5, 2.0, (3, M)).astype(np.float32)
    return x, w, b, scales


def _yardstick(O, form, x, w, b, scales, cuts3):
    """the oracle's sequential fp32 chain on the same data (the row-scaled forms: on x scaled in fp32, as the pre-fold pipeline did);
    returns (y_oracle, y64, D)"""
    M, K = x.shape
    xs = x.copy()
    Dx = np.abs(x.astype(np.float64))
    if FORMS[form]["form"] == 1:
        segs, _ = _seg_bounds(form, K, cuts3)
        rows = np.arange(M) % scales.shape[1]
        for i, (k0, k1) in enumerate(segs):
            xs[:, k0:k1] = (x[:, k0:k1] * scales[i, rows][:, None]).astype(np.float32)
            Dx[:, k0:k1] *= scales[i, rows].astype(np.float64)[:, None]
    y64 = ref64(form, x, w, b, 0, scales, cuts3)
    D = Dx @ np.abs(w.astype(np.float64)).T + np.abs(b.astype(np.float64))
    return O.linear(xs, w, b), y64, D


@pytest.mark.parametrize("shape,kind,form", ACC_CASES, ids=["%dx%dx%d-%s-%s" % (s + (k, f)) for s, k, f in ACC_CASES])
def test_accuracy_vs_float64(O, dev, shape, kind, form):
    """max and RMS of e = |y - y64| / (sum |x w| + |b|) within 1.5x those of O.linear's fp32 chain on the same data (the in-place row-scaled
    form: + 3u |y| / (sum |x w| + |b|) per element for its two or three extra roundings).
    Measured on the MI355X (ratio to the chain's max e / RMS e): the fp32 forms 0.09-1.10 / 0.10-1.02 — ri2 and the in-place row-scaled form
    are one k-ordered chain per output, like the oracle (1.0, up to 1.24 on the max for the in-place form on the wide data set); split-K and
    the row-invariant segments shorten the chains.  split3 0.07-0.73 / 0.07-0.66 (its auto K ranges shorten the chains too).  Absolute max e:
    0.75-4.2e-6 on all-positive data at K = 1024-4096 for the chain-like forms, <= 3e-7 on normal data."""
    M, K, N = shape
    x, w, b, scales = _acc_case(kind, M, K, N)
    cuts3 = _cuts(K)
    _, cuts = _seg_bounds(form, K, cuts3) if FORMS[form]["form"] == 1 else (None, [])
    yo, y64, D = _yardstick(O, form, x, w, b, scales, cuts3)
    y = run_form(form, x, w, b, scales=scales, cuts=cuts)
    em, er = _err(y, y64, D)
    om, orr = _err(yo, y64, D)
    extra = 3 * U * np.abs(y64) / D if "rsi" in form else 0.0
    emx = float((np.abs(y.astype(np.float64) - y64) / D - extra).max())
    print("ACC %s %s %-14s max e %.3g rms e %.3g | oracle max %.3g rms %.3g" % (shape, kind, form, em, er, om, orr))
    assert emx <= 1.5 * om and er <= 1.5 * orr + (float(np.sqrt((extra * extra).mean())) if "rsi" in form else 0.0), (em, er, om, orr)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. edge operands
# ---------------------------------------------------------------------------------------------------------------------------------------
EDGE_SHAPES = [(129, 300, 257), (7, 65, 3)]
EDGE_FORMS = [f for f in FORMS if f != "res"]
EDGE_CASES = [(s, f) for s in EDGE_SHAPES for f in EDGE_FORMS if _applies(f, *s)]


@pytest.mark.parametrize("shape,form", EDGE_CASES, ids=["%dx%dx%d-%s" % (s + (f,)) for s, f in EDGE_CASES])
def test_huge_finite_operands_stay_finite(O, dev, shape, form):
    """|x| in [3.3962e38, FLT_MAX] (bf16 rounding overflows there) against |w| <= 2^-30: finite, and as accurate as O.linear"""
    M, K, N = shape
    rng = np.random.default_rng(M + K)
    x = rng.standard_normal((M, K))
    for m in range(M):
        cols = rng.choice(K, min(4, K), replace=False)
        x[m, cols] = rng.choice([-1.0, 1.0], len(cols)) * rng.uniform(BF16_OVERFLOW, FLT_MAX, len(cols))
    x[0, :min(3, K)] = [BF16_OVERFLOW, -FLT_MAX, FLT_MAX][:min(3, K)]
    x = x.astype(np.float32)
    w = np.clip(rng.standard_normal((N, K)) * 2.0 ** -32, -2.0 ** -30, 2.0 ** -30).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    scales = rng.uniform(0.5, 1.0, (3, M)).astype(np.float32)  # (<= 1: the yardstick's pre-scaled x stays finite)
    cuts3 = _cuts(K)
    _, cuts = _seg_bounds(form, K, cuts3) if FORMS[form]["form"] == 1 else (None, [])
    yo, y64, D = _yardstick(O, form, x, w, b, scales, cuts3)
    y = run_form(form, x, w, b, scales=scales, cuts=cuts)
    assert np.isfinite(y).all(), "%d non-finite outputs" % (~np.isfinite(y)).sum()
    em, _ = _err(y, y64, D)
    om, _ = _err(yo, y64, D)
    assert em <= 1.5 * om + 8 * U, (em, om)


def _classes(y):
    return np.where(np.isnan(y), 0, np.where(np.isposinf(y), 1, np.where(np.isneginf(y), 2, 3)))


def _ref64_elementwise(form, x, w, b, relu, scales, cuts3):
    """float64 with IEEE inf / NaN semantics: an explicit elementwise sum (no BLAS)"""
    f = FORMS[form]
    M, K = x.shape
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if f["form"] == 1:
            segs, _ = _seg_bounds(form, K, cuts3)
            rows = np.arange(M) % scales.shape[1]
            y = 0.0
            for i, (k0, k1) in enumerate(segs):
                y = y + scales[i, rows].astype(np.float64)[:, None] * (x64[:, None, k0:k1] * w64[None, :, k0:k1]).sum(-1)
        else:
            y = (x64[:, None, :] * w64[None, :, :]).sum(-1)
        y = y + b.astype(np.float64)
        if f.get("res"):
            y = y + _residual(M, w.shape[0])
        return np.where(y < 0, 0.0, y) if relu else y  # ReLU: t < 0 ? 0 : t — NaN passes through


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape,form", EDGE_CASES, ids=["%dx%dx%d-%s" % (s + (f,)) for s, f in EDGE_CASES])
def test_inf_nan_operands_keep_the_float64_class(dev, shape, form, relu):
    """+-inf and NaN at chosen (row, k) of x and of w: every output is NaN / +inf / -inf / finite exactly when the float64 result is.
    Rows / columns cover inf against weights of both signs, +inf and -inf in one sum (NaN), inf against an exact zero weight (NaN), NaN,
    and weights whose bf16 correction planes are zero (+-1, +-2^e) or not."""
    M, K, N = shape
    rng = np.random.default_rng(3 * M + K)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = rng.standard_normal((N, K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    w[:, 1] = rng.choice([-1.0, 1.0, 0.5, -4.0], N)       # zero m / l planes
    w[0, 2] = 0.0                                           # inf x 0 -> NaN in column 0
    x[0, 1] = np.inf                                        # row 0: +inf against weights of both signs
    x[1, 2] = -np.inf                                       # row 1: -inf, and NaN in column 0 (w[0, 2] = 0)
    if M > 2:
        x[2, 0] = np.inf; x[2, K - 1] = -np.inf if K > 1 else np.inf   # row 2: inf - inf
    if M > 3:
        x[3, K // 2] = np.nan                               # row 3: NaN
    if M > 4:
        x[4, K - 1] = np.inf                                # row 4: inf in the last (partial) chunk
    if N > 2:
        w[2, K - 1] = np.inf                                # column 2: inf weight
    if N > 1:
        w[1, 0] = np.nan                                    # column 1: NaN weight
    if M > 5 and N > 2:
        x[5, K - 1] = 0.0                                   # 0 x inf -> NaN at (5, 2)
    scales = rng.uniform(0.5, 2.0, (3, M)).astype(np.float32)
    cuts3 = _cuts(K)
    _, cuts = _seg_bounds(form, K, cuts3) if FORMS[form]["form"] == 1 else (None, [])
    y = run_form(form, x, w, b, relu=relu, scales=scales, cuts=cuts)
    y64 = _ref64_elementwise(form, x, w, b, relu, scales, cuts3)
    cg, cr = _classes(y), _classes(y64)
    bad = np.argwhere(cg != cr)
    names = ["NaN", "+inf", "-inf", "finite"]
    assert bad.size == 0, "%d outputs in the wrong class, first at %s: %s (%r), float64 %s" % (
        len(bad), tuple(bad[0]), names[cg[tuple(bad[0])]], float(y[tuple(bad[0])]), names[cr[tuple(bad[0])]])
    fin = cr == 3
    assert np.isfinite(y64[fin]).all()


SUBNORMAL_FORMS = ["product", "kch8", "split5", "ri1", "ri2", "rs3_rsi", "rs3_fold", "split3_auto"]


@pytest.mark.parametrize("form", SUBNORMAL_FORMS)
def test_subnormal_operands(O, dev, form):
    """x in [2^-149, 2^-126), w = +-2^20 * [1, 2): the fp32 forms keep fp32 subnormals (hipcc's default denorm mode; MFMA C/D never flush):
    as accurate as the fp32 chain.  The three-plane split cannot hold an fp32 subnormal below bf16's 2^-133 grid: each x is carried to within
    2^-134 absolutely (mpn.h, fc_arith), so its bound is that plus the chain's: |y - y64| <= 2^-134 sum_k |w_k| + 1.5 x O.linear's error.
    Measured on the MI355X: the fp32 forms' max e 1.4-4.2e-7 beside the chain's 4.4e-7 (nothing flushed); split3 max |y - y64| = 2^-137.1
    sum_k |w_k| — v_cvt_pk_bf16_f32 and the bf16 MFMA keep bf16 subnormals (a flush would cost up to 2^-126 sum_k |w_k|)."""
    M, K, N = 129, 300, 129
    rng = np.random.default_rng(149)
    x = (rng.choice([-1.0, 1.0], (M, K)) * 2.0 ** rng.uniform(-149, -126, (M, K))).astype(np.float32)
    w = (rng.choice([-1.0, 1.0], (N, K)) * 2.0 ** 20 * rng.uniform(1, 2, (N, K))).astype(np.float32)
    b = np.zeros(N, np.float32)
    scales = np.ones((3, M), np.float32)
    cuts3 = _cuts(K)
    _, cuts = _seg_bounds(form, K, cuts3) if FORMS[form]["form"] == 1 else (None, [])
    assert (np.abs(x) < 2.0 ** -126).all() and (x != 0).all()
    yo, y64, D = _yardstick(O, form, x, w, b, scales, cuts3)
    y = run_form(form, x, w, b, scales=scales, cuts=cuts)
    d = np.abs(y.astype(np.float64) - y64)
    do = np.abs(yo.astype(np.float64) - y64)
    W1 = np.abs(w.astype(np.float64)).sum(1)[None, :]
    print("SUBNORMAL %-12s max |y - y64| / sum|w| = %.3g (2^%.1f); max e %.3g, oracle %.3g" % (
        form, (d / W1).max(), np.log2(max((d / W1).max(), 1e-300)), (d / D).max(), (do / D).max()))
    if FORMS[form]["form"] == 2:
        assert (d <= 2.0 ** -134 * W1 + 1.5 * do.max() + 2.0 ** -149).all()
    else:
        assert (d / D).max() <= 1.5 * (do / D).max() + U


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the plane split
# ---------------------------------------------------------------------------------------------------------------------------------------
def _rne_bf16(x):
    """fp32 -> bf16 bits, round to nearest even (what v_cvt_pk_bf16_f32 does); finite values only"""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bf(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def _split_host(x):
    """the split as specified: h = RNE(x) (clamped to +-0x7F7F where that overflows a finite x), m = RNE(x - h), l = RNE(x - h - m)"""
    x = np.asarray(x, np.float32)
    h = _rne_bf16(x)
    ov = (h & 0x7FFF) == 0x7F80
    h = np.where(ov, h - 1, h).astype(np.uint16)
    r = (x - _bf(h)).astype(np.float32)
    m = _rne_bf16(r)
    l = _rne_bf16((r - _bf(m)).astype(np.float32))
    return h, m, l


def _planes_dev(x):
    n = len(x)
    n8 = (n + 7) // 8 * 8
    xp = np.zeros(n8, np.float32)
    xp[:n] = x
    xd = torch.from_numpy(xp).cuda()
    out = torch.zeros(3 * n8, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    assert _dbg().mpn_debug_split3_planes(_ptr(xd), n8, _ptr(out)) == 0, _dbg().mpn_last_error()
    p = out.cpu().numpy().view(np.uint16).reshape(3, n8)[:, :n]
    return p[0], p[1], p[2]


def _plane_inputs():
    f = np.float32
    bmax = float(_bf(np.uint16(0x7F7F)))
    special = [0.0, 2.0 ** -149, 2.0 ** -126, 1.0, bmax, float(np.nextafter(f(bmax), f(np.inf))), float(np.nextafter(f(BF16_OVERFLOW), f(0))),
               BF16_OVERFLOW, float(np.nextafter(f(BF16_OVERFLOW), f(np.inf))), FLT_MAX, 2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -135,
               1 + 2.0 ** -23, 1 - 2.0 ** -24, 1 + 2.0 ** -8 + 2.0 ** -16, 2.0 ** -110 * (1 + 2.0 ** -23), 65504.0, 1.0 / 3]
    rng = np.random.default_rng(7)
    rand = rng.integers(0, 0x7F800000, 4096, dtype=np.uint32).view(np.float32).astype(np.float64)  # every finite magnitude, uniform in bits
    v = np.concatenate([special, rand, rng.uniform(BF16_OVERFLOW, FLT_MAX, 64)])
    v = np.concatenate([v, -v, [-0.0]]).astype(np.float32)
    return v


def test_plane_split_is_exact_and_unchanged_below_the_overflow(dev):
    """h + m + l == x exactly (float64) for every finite fp32 x down to 2^-110 (the l plane's grid reaches x's last bit) and for every x on
    bf16's own 2^-133 grid (the min normal among them); below that |x - (h + m + l)| <= 2^-134 (an fp32 subnormal off bf16's grid: the
    only inexact split).  Bit for bit the host RNE split for |x| < 3.3962e38; from there to FLT_MAX h = +-0x7F7F and the split is exact."""
    x = _plane_inputs()
    h, m, l = _planes_dev(x)
    eh, em, el = _split_host(x)
    bad = np.flatnonzero((h != eh) | (m != em) | (l != el))
    assert bad.size == 0, "planes differ from the host split at x = %r: got %s, want %s" % (
        float(x[bad[0]]), [hex(v[bad[0]]) for v in (h, m, l)], [hex(v[bad[0]]) for v in (eh, em, el)])
    s = _bf(h).astype(np.float64) + _bf(m).astype(np.float64) + _bf(l).astype(np.float64)
    x64 = x.astype(np.float64)
    on_grid = np.abs(x64) >= 2.0 ** -110
    on_grid |= (x64 / 2.0 ** -133) == np.round(x64 / 2.0 ** -133)
    assert np.array_equal(s[on_grid], x64[on_grid])
    assert (np.abs(s - x64) <= 2.0 ** -134).all()
    assert np.isfinite(_bf(h)).all()
    big = np.abs(x64) >= BF16_OVERFLOW
    assert big.sum() > 100 and ((h[big] & 0x7FFF) == 0x7F7F).all()
    # -0.0 splits into -0.0 and zeros; x = 0 gives three zero planes
    assert h[-1] == 0x8000 and m[-1] & 0x7FFF == 0 and l[-1] & 0x7FFF == 0


def test_plane_split_of_non_finite_values(dev):
    """+-inf and NaN: h carries the value, m = l = +-0 (x - h would be inf - inf = NaN in the correction planes)"""
    x = np.array([np.inf, -np.inf, np.nan, -np.nan, 1.0, np.inf, 0.0, np.nan], np.float32)
    h, m, l = _planes_dev(x)
    hf = _bf(h)
    assert np.isposinf(hf[0]) and np.isneginf(hf[1]) and np.isnan(hf[2]) and np.isnan(hf[3]) and np.isposinf(hf[5]) and np.isnan(hf[7])
    nf = ~np.isfinite(x)
    assert ((m[nf] & 0x7FFF) == 0).all() and ((l[nf] & 0x7FFF) == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. row invariance
# ---------------------------------------------------------------------------------------------------------------------------------------
INV_FORMS = ["ri1", "ri2", "rs3_rsi", "rs3_fold", "split3_auto", "split3_3"]


@pytest.mark.parametrize("K,N", [(4096, 129), (25088, 4096), (300, 4097)])
@pytest.mark.parametrize("form", INV_FORMS)
def test_row_invariant_forms_do_not_depend_on_the_row_count(dev, form, K, N):
    """the first m rows of a 1001-row call are bit-identical to an m-row call (m = 7, 129, 257) — normal data, so every bit counts"""
    rng = np.random.default_rng(K + N)
    x = rng.standard_normal((1001, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    scales = rng.uniform(0.5, 2.0, (3, 1001)).astype(np.float32)
    _, cuts = _seg_bounds(form, K, _cuts(K)) if FORMS[form]["form"] == 1 else (None, [])
    full = run_form(form, x, w, b, scales=scales, cuts=cuts)
    for m in (7, 129, 257):
        part = run_form(form, x[:m], w, b, scales=scales[:, :m], cuts=cuts)
        assert np.array_equal(part.view(np.uint32), full[:m].view(np.uint32)), (form, m)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. zero and pad row scales (MultiPathNet's mix GEMM)
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad_scale", [1.0, 0.0])
@pytest.mark.parametrize("n_roi,packed", [(37, 1), (125, 1), (37, 0), (130, 0)])
@pytest.mark.parametrize("n_seg", [1, 2, 3])
@pytest.mark.parametrize("rsi", [1, 0])
def test_rowscaled_pad_rows_stay_finite(O, dev, rsi, n_seg, n_roi, packed, pad_scale):
    """The mix GEMM's rows are (bin, roi): per bin the real ROIs, then zero pad rows up to 8 (packed) or 128 (unpacked), whose scale is what
    l2norm_scale_rows_kernel writes (1) — or 0, outside the contract (dense.h GemmRowScale), which the in-place form must survive too.
    Every stored row of the raw C8 output is finite, the gap rows of the packed scatter are never written, the in-place (RSI) and
    running-total (FOLD) forms agree to rounding on the real rows, and both are within the accuracy bound of float64."""
    bins, K, N = 5, 320, 131
    bin_rows = (n_roi + 7) // 8 * 8 if packed else (n_roi + 127) // 128 * 128
    M = bins * bin_rows
    rng = np.random.default_rng(n_roi + 1000 * n_seg)
    x = np.abs(rng.standard_normal((bins, bin_rows, K))).astype(np.float32)
    x[:, n_roi:] = 0.0
    x = x.reshape(M, K)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    scales = rng.uniform(0.01, 0.1, (3, bin_rows)).astype(np.float32)  # rs_mod = rows per bin: the scale of (bin, roi) is scale[roi]
    scales[:, n_roi:] = pad_scale
    form = "rs%d_%s%s" % (n_seg, "rsi" if rsi else "fold", "_packed" if packed else "")
    cuts3 = _cuts(K)
    _, cuts = _seg_bounds(form, K, cuts3)
    y, raw, (nb, br, omp) = run_form(form, x, w, b, scales=scales, cuts=cuts, raw=True)
    real = (np.arange(M) % bin_rows) < n_roi
    if packed:
        r = raw[:, :N].reshape(nb, omp, N)
        assert np.isfinite(r[:, :br]).all(), "non-finite stored rows: %s" % np.argwhere(~np.isfinite(r[:, :br]))[:4]
        assert np.isnan(r[:, br:]).all(), "the packed scatter wrote into the gap between bins"
    else:
        assert np.isfinite(raw[:M, :N]).all(), "non-finite stored rows: %s" % np.argwhere(~np.isfinite(raw[:M, :N]))[:4]
    # the pad rows' outputs: an unscaled zero row, i.e. the bias
    assert np.array_equal(y[~real], np.broadcast_to(b, y[~real].shape))
    yo, y64, D = _yardstick(O, form, x, w, b, np.ascontiguousarray(scales), cuts3)
    e = np.abs(y.astype(np.float64) - y64)[real] / D[real]
    eo = np.abs(yo.astype(np.float64) - y64)[real] / D[real]
    assert e.max() <= 1.5 * eo.max() + 3 * U


@pytest.mark.parametrize("n_roi,mp", [(37, 40), (37, 128), (125, 128), (8, 8)])
def test_normalising_pool_writes_finite_nonzero_scales_on_every_row(dev, n_roi, mp):
    """The producer side: roi_pool_pm_rmq with d_scale_out (nn.Normalize(2) x mul folded into the consumer GEMM) writes a finite non-zero
    scale for every row up to rs_mod — the real ROIs' mul / ||pooled|| and 1 for the pad rows"""
    rng = np.random.default_rng(n_roi)
    Cc, H, W = 64, 19, 23
    feat = torch.from_numpy(rng.standard_normal((Cc, H, W)).astype(np.float32)).cuda()
    c = rng.uniform([0, 0], [W * 16, H * 16], (n_roi, 2))
    wh = rng.uniform(16, 200, (n_roi, 2))
    rois = np.zeros((n_roi, 5), np.float32)
    rois[:, 1:] = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, [W * 16 - 1, H * 16 - 1] * 2)
    rois[0, 1:] = [1000, 1000, 1000, 1000]  # a ROI outside the map: empty bins, pooled row all zero
    rd = torch.from_numpy(rois).cuda()
    out = torch.empty(mp, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    lib = _dbg()
    assert lib.mpn_debug_l2norm_row_scales(_ptr(feat), Cc, H, W, _ptr(rd), 5, n_roi, 7, 7, C.c_float(1 / 16), mp, C.c_float(1000.0), _ptr(out)) == 0, \
        lib.mpn_last_error()
    s = out.cpu().numpy()
    assert np.isfinite(s).all() and (s != 0).all(), s
    assert (s[:n_roi] > 0).all() and (s[n_roi:] == 1.0).all()


def test_mpnet_with_ragged_roi_count_matches_the_oracle(O, dev):
    """At pipeline level, 37 ROIs (packed bins of 40 rows: three pad rows per bin): in-place and running-total row scales agree to rounding
    and both are within the path's 1e-4 of the oracle — the pad-row scale changes no real row"""
    from multipathnet_amd import models
    cfg = [16, 32, "P", 32, 64, "P", 64, 96, "P", 128, "P", 384]
    H, W, N, Cn, K = 150, 250, 37, 9, 3
    P = models.synthetic_mpnet_params(cfg, pooled=7, fc_dim=256, n_classes=Cn, n_integral=K, seed=11)
    rng = np.random.default_rng(37)
    im_np = rng.random((3, H, W), dtype=np.float32)
    c = rng.uniform([1, 1], [W, H], (N, 2))
    wh = np.exp(rng.uniform(np.log(12), np.log(min(W, H)), (N, 2)))
    bx_np = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 1, [W, H, W, H]).astype(np.float32)
    im, bx = torch.from_numpy(im_np).to(dev), torch.from_numpy(bx_np).to(dev)
    outs = []
    for rsi in (1, 0):
        with hooks(gemm_rsi=rsi):
            net = models.MultiPathNet(P, cfg=cfg, pooled=7, spatial_scale=1 / 16, max_h=H, max_w=W, max_rois=N)
            s1, b1 = net.detect(im, bx)
            torch.cuda.synchronize()
            assert torch.isfinite(s1).all() and torch.isfinite(b1).all()
            outs.append((s1.clone(), b1.clone()))
            del net
    assert float((outs[0][0] - outs[1][0]).abs().max()) < 2e-6 and float((outs[0][1] - outs[1][1]).abs().max()) < 1e-3
    Pn = _np_tree(P)
    taps = {}
    O.vgg_trunk(O.image_transform(im_np, **O.ROSS), Pn["conv_w"], Pn["conv_b"], cfg, taps=taps)
    ref_scores, _ = O.mpnet_head([taps["conv5"], taps["conv4"], taps["conv3"]], O.project_im_rois(bx_np, 1.0), Pn)
    assert np.abs(outs[0][0].cpu().numpy() - ref_scores).max() < 1e-4


def _np_tree(v):
    if isinstance(v, dict):
        return {k: _np_tree(x) for k, x in v.items()}
    if isinstance(v, list):
        return [_np_tree(x) for x in v]
    return v.numpy() if hasattr(v, "numpy") else v
