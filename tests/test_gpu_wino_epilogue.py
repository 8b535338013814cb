"""The Winograd kernel's epilogue paths (dense.hip, conv3x3_wino_kernel), one layer at a time through mpn_debug_conv3x3_form.

The epilogue has one copy per finish: interior blocks (all 64 tiles inside the map: no store predicate) finishing a full map, a pooled map
only (2x2 maximum first, then ONE bias add and ReLU), a tap layer or a split-K slab, and the predicated copy for edge blocks; the K loop's
first chunk starts from a zero C operand (one copy per first-buffer parity; a one-chunk block zeroes its accumulators).  The shapes are the
smallest that reach each of them:
  maps      16x16 / 8x32 (exactly one interior block of the 16x16-px / 8x32-px geometry), 32x64 (interior blocks only), 17x33 (interior and
            edge blocks in one launch, odd pooled size 9x17), 5x7 (edge blocks only), 31x18 (odd height; an x edge for 8x32-px blocks only)
  channels  Cin 8 (one chunk), 16, 24 (both first-buffer parities); Cout 8, 64, 72 (the second cout tile has channel blocks past out_cb)
  modes     full map, pooled only, both; ReLU on / off; wino_tc 8 / 16; conv_split 0 (the cost model's plan: it cuts a lone block's 3
            chunks in 3), 1 (un-split: the base the others are compared with), 2 (uniform split), -2 (tail split over the second half of
            the tiles).
Every call asserts the plan that ran (mpn_debug_conv3x3_last_plan): the Winograd form, the block geometry and the split (conv_split 0: that
the recorded split is a consistent one, since which one is the cost model's business).

Expectations (none depends on the code under test):
  1 exact    integer operands |x| <= 1, |w| <= 1, |b| <= 8: sum |x w| + |b| <= 9 x 24 + 8 = 224 <= 256 and the Winograd transforms hold
             multiples of 1/4 (test_gpu_trunk_conv_numerics.py's argument), so every fp32 intermediate is exact: full and pooled maps equal the
             float64 convolution (and its ceil-mode 2x2 max) bit for bit in every mode, geometry and split;
  2 pooled   He-scaled random data: a tap-layer call's pooled map is maxpool2x2_c8p (kind 2) of that call's own full map bit for bit, the
             pooled-only call gives the same pooled bits, a second run the same bits.  A split that does not change the summation (one
             chunk: the split clamps to 1; the tail split's tiles before tail_first) equals the un-split call bit for bit; a split that
             re-groups the channel sum cannot on random data (it is bit-equal in tier 1, where every sum is exact) and stays within the
             trunk numerics test's re-grouping bound 2 x 9 (Cin8 + 9) 2^-24 T;
  3 stores   the buffers are pre-filled with the sentinel NaN: outside the H x W interior of every plane it survives, the pad lanes of the
             last channel block are +0.0 and a buffer the mode does not ask for is untouched (the trunk numerics test's rule, _check_layout);
  4 edge     NaN, +-inf and a subnormal in an interior tile, an edge tile, the first and the last channel: what the trunk numerics test pins
             for the Winograd form (a non-finite input reaches only its tiles' patches, a non-finite float64 output is non-finite,
             ReLU(NaN) = 0, a pooling window ignores its NaNs and a window of NaNs gives -inf), in every finish.
"""
import functools

import numpy as np
import pytest
import torch

import test_gpu_trunk_conv_numerics as T

pytestmark = pytest.mark.gpu

FULL, POOLED, BOTH = T.FULL, T.POOLED, T.BOTH
MAPS = [(16, 16), (8, 32), (32, 64), (17, 33), (5, 7), (31, 18)]
CINS = [8, 16, 24]
COUTS = [8, 64, 72]
SPLITS = [1, 0, 2, -2]   # 1 first: the un-split base
TCS = [8, 16]


def cdiv(a, b):
    return (a + b - 1) // b


def want_plan(Cin, H, W, Cout, tc, split):
    """(variant, wino_tc, splits, chunks_per_split, tail_first, tail_splits, tail_cps, reduce ran) of a forced geometry / split"""
    nch = cdiv(Cin, 8)
    th, tw = (8, 32) if tc == 16 else (16, 16)
    n_ct = cdiv(Cout, 64)
    blocks = n_ct * cdiv(H, th) * cdiv(W, tw)
    if split > 0:
        cps = cdiv(nch, min(split, nch))
        s = cdiv(nch, cps)
        return (7, tc, s, cps, 0, 0, 0, int(s > 1))
    if split < 0:
        S, first = min(-split, nch), (blocks // 2 // n_ct) * n_ct
        if S > 1 and 0 < first < blocks:
            tcps = cdiv(nch, S)
            if cdiv(nch, tcps) >= 2:
                return (7, tc, 1, nch, first, cdiv(nch, tcps), tcps, 1)
    return (7, tc, 1, nch, 0, 0, 0, 0)


def launch(x, w, b, relu, mode, tc, split, kind=T.CONV):
    """ONE call; returns (full, pooled) as T.Raw (None where the mode does not ask for the buffer), after asserting the plan that ran and
    that the buffer the mode does not ask for still holds the sentinel"""
    lib = T._dbg()
    Cin, H, W = x.shape
    Cout = Cin if kind == T.POOL else w.shape[0]
    PH, PW = (H + 1) // 2, (W + 1) // 2
    fbuf, fhp, fwp = T._sentinel_buf(lib, Cout, H, W)
    pbuf, php, pwp = T._sentinel_buf(lib, Cout, PH, PW)
    xd, wd, bd = T._dev(x), T._dev(w), T._dev(b)
    want_f, want_p = mode in (FULL, BOTH), mode in (POOLED, BOTH)
    torch.cuda.synchronize()
    with T._knobs(lib, conv_variant=0, wino_tc=tc, conv_split=split):
        rc = lib.mpn_debug_conv3x3_form(T._ptr(xd), Cin, H, W, T._ptr(wd), T._ptr(bd), Cout, int(relu), kind, 1, 0,
                                        T._ptr(fbuf) if want_f else None, T._ptr(pbuf) if want_p else None)
    assert rc == 0, lib.mpn_last_error().decode()
    if kind == T.CONV:
        want = want_plan(Cin, H, W, Cout, tc, split)
        if split == 0:   # the cost model's choice: any consistent split of the Winograd form in the forced geometry
            got, nch = T.last_plan(), cdiv(Cin, 8)
            assert got[:2] == (7, tc) and got[2] == cdiv(nch, got[3]) and got[7] == int(got[2] > 1 or got[5] > 1), got
            assert (got[4:7] == (0, 0, 0)) or (got[2] == 1 and got[4] > 0 and got[5] == cdiv(nch, got[6]) > 1), got
            want = got
        assert T.last_plan() == want, "Cin %d %dx%d Cout %d tc %d split %d launched plan %s, meant %s" % (Cin, H, W, Cout, tc, split, T.last_plan(), want)
    full = T.Raw(fbuf.cpu().numpy().view(np.uint32), Cout, H, W, fhp, fwp)
    pooled = T.Raw(pbuf.cpu().numpy().view(np.uint32), Cout, PH, PW, php, pwp)
    if not want_f:
        assert (full.w == T.SENT).all(), "the full-map buffer was written in mode %s" % mode
    if not want_p:
        assert (pooled.w == T.SENT).all(), "the pooled buffer was written in mode %s" % mode
    return (full if want_f else None), (pooled if want_p else None)


def _rng(*key):
    return np.random.default_rng([557] + [int(k) & 0xFFFF for k in key])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1 + 3: exact tier, stores stay inside
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_case(H, W, Cin, Cout):
    """operands and the float64 references (no ReLU / ReLU), computed once and shared by every geometry, split and mode"""
    rng = _rng(H, W, Cin, Cout)
    x = rng.integers(-1, 2, (Cin, H, W)).astype(np.float32)
    w = rng.integers(-1, 2, (Cout, Cin, 3, 3)).astype(np.float32)
    b = rng.integers(-8, 9, Cout).astype(np.float32)
    bound = T.ref64(x, w, b, absolute=True).max()
    assert bound <= 256
    y64 = [T.ref64(x, w, b, relu=r).astype(np.float32) for r in (0, 1)]
    return x, w, b, y64


@pytest.mark.parametrize("tc", TCS)
@pytest.mark.parametrize("hw", MAPS, ids=lambda hw: "%dx%d" % hw)
def test_exact_and_stores(dev, hw, tc):
    H, W = hw
    for Cin in CINS:
        for Cout in COUTS:
            x, w, b, y64 = exact_case(H, W, Cin, Cout)
            for split in SPLITS:
                for relu in (0, 1):
                    for mode in (FULL, POOLED, BOTH):
                        name = "%dx%d c%d o%d tc%d split %d relu %d" % (H, W, Cin, Cout, tc, split, relu)
                        full, pooled = launch(x, w, b, relu, mode, tc, split)
                        T._check_exact(name, mode, full, pooled, y64[relu])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2: pooled consistency on random data
# ---------------------------------------------------------------------------------------------------------------------------------------
def he_operands(H, W, Cin, Cout):
    rng = _rng(H, W, Cin, Cout, 2)
    x = rng.standard_normal((Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) * np.sqrt(2.0 / (Cin * 9))).astype(np.float32)
    b = (rng.standard_normal(Cout) * 0.1).astype(np.float32)
    return x, w, b


def _tail_done_by_own_block(H, W, tc, tail_first, n_ct):
    """[H, W] mask of the pixels whose tile a tail split leaves to its own block (tile index < tail_first / n_ct)"""
    th, tw = (8, 32) if tc == 16 else (16, 16)
    ty, tx = np.arange(H)[:, None] // th, np.arange(W)[None, :] // tw
    return (ty * cdiv(W, tw) + tx) < tail_first // n_ct


@pytest.mark.parametrize("tc", TCS)
@pytest.mark.parametrize("hw", MAPS, ids=lambda hw: "%dx%d" % hw)
def test_pooled_consistency(dev, hw, tc):
    H, W = hw
    for Cin, Cout in ((8, 72), (16, 8), (24, 72)):
        x, w, b = he_operands(H, W, Cin, Cout)
        nch = cdiv(Cin, 8)
        tol = 18 * (nch * 8 + 9) * 2.0 ** -24 * (T._wino_term_bound(x, w) + np.abs(b.astype(np.float64))[:, None, None])
        for relu in (0, 1):
            base = None
            for split in SPLITS:
                tag = "%dx%d c%d o%d tc%d split %d relu %d" % (H, W, Cin, Cout, tc, split, relu)
                full, pooled = launch(x, w, b, relu, BOTH, tc, split)
                y, p = full.interior(), pooled.interior()
                own = launch(y, None, None, 0, POOLED, 0, 0, kind=T.POOL)[1].interior()
                assert np.array_equal(T._bits(p), T._bits(own)), "%s: the fused pool differs from maxpool2x2_c8p of the call's own full map" % tag
                only = launch(x, w, b, relu, POOLED, tc, split)[1].interior()
                assert np.array_equal(T._bits(only), T._bits(p)), "%s: the pooled-only call differs from the tap-layer call" % tag
                if split == 1:
                    base = y
                    again = launch(x, w, b, relu, BOTH, tc, split)
                    assert np.array_equal(again[0].w, full.w) and np.array_equal(again[1].w, pooled.w), "%s: a second run differs" % tag
                    continue
                plan = T.last_plan() if split == 0 else want_plan(Cin, H, W, Cout, tc, split)
                if plan[7] == 0:   # the split clamped to the un-split launch
                    assert np.array_equal(T._bits(y), T._bits(base)), "%s: differs from the un-split call" % tag
                    continue
                if plan[5] > 1:    # tail split: the tiles before tail_first are finished by their own un-split block
                    m = _tail_done_by_own_block(H, W, tc, plan[4], cdiv(Cout, 64))
                    assert m.any()
                    assert np.array_equal(T._bits(y[:, m]), T._bits(base[:, m])), "%s: tiles before tail_first differ from the un-split call" % tag
                d = np.abs(y.astype(np.float64) - base.astype(np.float64))
                assert (d <= tol).all(), "%s: |split - un-split| %g above the re-grouping bound %g" % (tag, d.max(), tol.flat[np.argmax(d - tol)])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4: edge values
# ---------------------------------------------------------------------------------------------------------------------------------------
EDGE_H, EDGE_W, EDGE_CIN, EDGE_COUT = 17, 33, 24, 72


def _edge_spots():
    """(channel, y, x, value): an interior tile of the interior block (both geometries: rows < 8, columns < 16), the edge blocks' last row
    and column, the first and the last channel"""
    H, W, Cin = EDGE_H, EDGE_W, EDGE_CIN
    return [(0, 3, 5, np.nan), (Cin - 1, 4, 10, np.inf), (0, H - 1, W - 1, np.nan), (Cin - 1, H - 1, 0, -np.inf), (0, 0, W - 1, np.inf)]


def _reach():
    H, W = EDGE_H, EDGE_W
    m = np.zeros((H, W), bool)
    ty, tx = (np.arange(H) & ~1)[:, None], (np.arange(W) & ~1)[None, :]
    for _, iy, ix, _ in _edge_spots():
        m |= (ty - 1 <= iy) & (iy <= ty + 2) & (tx - 1 <= ix) & (ix <= tx + 2)
    return m


@functools.lru_cache(maxsize=None)
def edge_case():
    x0, w, b = he_operands(EDGE_H, EDGE_W, EDGE_CIN, EDGE_COUT)
    x0[EDGE_CIN // 2, 2, 2] = 1.0e-40     # subnormals: an interior tile and an edge tile
    x0[0, EDGE_H - 1, EDGE_W // 2] = -3.0e-39
    x = x0.copy()
    for ch, yy, xx, v in _edge_spots():
        x[ch, yy, xx] = v
    y64 = T.ref_elementwise(x, w, b)
    return x0, x, w, b, y64


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("tc", TCS)
def test_edge_values(dev, tc, split):
    x0, x, w, b, y64 = edge_case()
    reach = _reach()
    assert np.isnan(y64).any() and np.isinf(y64).any() and not reach.all() and np.isfinite(y64[:, ~reach]).all()
    y = launch(x, w, b, 0, FULL, tc, split)[0].interior()
    y0 = launch(x0, w, b, 0, FULL, tc, split)[0].interior()
    assert np.isfinite(y0).all()
    assert np.array_equal(T._bits(y[:, ~reach]), T._bits(y0[:, ~reach])), "a non-finite input changed outputs outside its tiles' patches"
    assert not np.isfinite(y[~np.isfinite(y64)]).any(), "a non-finite float64 output came out finite"
    assert np.isnan(y).any()
    assert T.RELU_NAN[7] == 0.0
    for relu in (0, 1):
        full, pooled = launch(x, w, b, relu, BOTH, tc, split)
        yr, p = full.interior(), pooled.interior()
        if relu:
            assert not np.isnan(yr).any(), "ReLU(NaN) must be 0 on every Winograd launch; %d NaN outputs" % int(np.isnan(yr).sum())
            assert (yr[np.isnan(y)] == 0.0).all()
            assert np.array_equal(T._bits(yr[:, ~reach]), T._bits(np.where(y0 < 0, 0.0, y0)[:, ~reach]))
        else:
            assert np.array_equal(T._bits(yr), T._bits(y)), "the tap-layer call's full map differs from the full-map call's"
            assert (T.pool_ref(yr) == -np.inf).any(), "no all-NaN (or -inf) window was produced"
        assert not np.isnan(p).any(), "relu %d: %d pooled outputs are NaN" % (relu, int(np.isnan(p).sum()))
        assert np.array_equal(T._bits(p), T._bits(T.pool_ref(yr))), "relu %d: the fused pool differs from the rule" % relu
        only = launch(x, w, b, relu, POOLED, tc, split)[1].interior()
        assert np.array_equal(T._bits(only), T._bits(p)), "relu %d: the pooled-only call differs from the tap-layer call" % relu
