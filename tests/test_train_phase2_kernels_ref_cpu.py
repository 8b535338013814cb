"""The restatements and input sets of tests/test_gpu_train_phase2_kernels_numerics.py, checked without a GPU:
the generalised Normalize-backward order against its c5 % 8 == 0 form and against float64 autograd, the fma emulation against exact
integer and rational arithmetic, every input set against the condition its tier rests on, the chain restatement of the gather against
tests/train_conv_kernels_np.py's ordered sum."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_conv_kernels_np as K  # noqa: E402
import train_kernels_np as R  # noqa: E402
import train_phase2_kernels_np as Q  # noqa: E402
import train_phase2_np as P2  # noqa: E402

F32, F64 = np.float32, np.float64
NT = P2.NORM_THREADS
CASE_IDS = ["C%d_PP%d_B%d_Mp%d" % c for c in Q.NORM_CASES]


# ---- the c5 % 8 == 0 forms as they stood before the generalisation ------------------------------------------------------------------
def _old_entry_order(a):
    B, c5, PP = a.shape
    assert c5 % 8 == 0
    e = a.reshape(B, c5 // 8, 8, PP).transpose(0, 1, 3, 2).reshape(B, -1)
    L = -(-e.shape[1] // NT)
    pad = np.zeros((B, L * NT), a.dtype)
    pad[:, :e.shape[1]] = e
    return pad.reshape(B, L, NT)


def _old_fma_sum(a, b):
    A, Bv = _old_entry_order(np.asarray(a, F32)).astype(F64), _old_entry_order(np.asarray(b, F32)).astype(F64)
    part = np.zeros((A.shape[0], NT), F32)
    for l in range(A.shape[1]):
        part = (A[:, l] * Bv[:, l] + part.astype(F64)).astype(F32)
    h = NT // 2
    while h >= 1:
        part = (part[:, :h] + part[:, h:2 * h]).astype(F32)
        h //= 2
    return part[:, 0]


@pytest.mark.parametrize("C,PP,B", [(48, 49, 5), (40, 49, 3), (8, 32, 3), (8, 1, 2), (512, 49, 1)])
def test_generalised_order_is_the_old_one_at_multiples_of_8(C, PP, B):
    rng = np.random.default_rng([C, PP, B])
    x, y, g = (R.draw(rng, (B, C, PP)) for _ in range(3))
    vals, real = P2._entry_order(x)
    assert real.reshape(-1)[:C * PP].all() and not real.reshape(-1)[C * PP:].any()
    assert np.array_equal(vals, _old_entry_order(x))
    assert np.array_equal(R.bits(P2._fma_sum(x, y)), R.bits(_old_fma_sum(x, y)))
    old = (F32(P2.MUL) / np.sqrt((_old_fma_sum(x, x) + F32(1e-10)).astype(F32)).astype(F32)).astype(F32)[:, None, None] * \
        (g - (y * (_old_fma_sum(y, g) / F32(F32(P2.MUL) * F32(P2.MUL))).astype(F32)[:, None, None]).astype(F32)).astype(F32)
    assert np.array_equal(R.bits(P2.normalize_backward_f32(x, y, g)), R.bits(old.astype(F32)))
    L = -(-(C * PP) // NT)   # the old bound's chain length
    assert P2.norm_entries(C, PP) == C * PP and -(-P2.norm_entries(C, PP) // NT) == L


def test_entry_order_with_pad_lanes():
    """C = 11, PP = 3: entry e = ((c / 8) * PP + bin) * 8 + c % 8; block 1 has lanes 0..2 real, 3..7 pad"""
    a = np.arange(2 * 11 * 3, dtype=F32).reshape(2, 11, 3) + 1
    vals, real = P2._entry_order(a)
    E = P2.norm_entries(11, 3)
    assert E == 48 and vals.shape == (2, 1, NT)
    for c in range(16):
        for b in range(3):
            e = ((c // 8) * 3 + b) * 8 + c % 8
            assert real[0, e] == (c < 11)
            assert (vals[:, 0, e] == (a[:, c, b] if c < 11 else 0)).all()
    assert not real[0, E:].any() and real.sum() == 33
    # the bound's chain length counts the slots of the walk, pad lanes included
    assert -(-P2.norm_entries(33, 8) // NT) == 2 and -(-(33 * 8) // NT) == 2 and P2.norm_entries(33, 8) == 320
    assert -(-P2.norm_entries(9, 29) // NT) == 2 and -(-(9 * 29) // NT) == 2
    assert -(-P2.norm_entries(9, 16) // NT) == 1 and -(-P2.norm_entries(9, 17) // NT) == 2 and -(-(9 * 17) // NT) == 1


@pytest.mark.parametrize("C,PP", [(9, 7), (33, 8), (44, 49), (3, 1)])
def test_closed_form_is_float64_autograd(C, PP):
    rng = np.random.default_rng([C, PP, 5])
    for mul in (1000.0, 0.37):
        x = rng.normal(0, 1, (4, C, PP))
        x[1] = 0.0
        g = rng.normal(0, 1, x.shape)
        xt = torch.as_tensor(x).requires_grad_(True)
        yt = xt * mul / torch.sqrt((xt * xt).sum((1, 2), keepdim=True) + 1e-10)
        yt.backward(torch.as_tensor(g))
        got, ref = P2.normalize_backward64(x, yt.detach().numpy(), g, mul), xt.grad.numpy()
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


# ---- the fma emulation ---------------------------------------------------------------------------------------------------------------
def _round24(t):
    """int64 -> the nearest integer with at most 24 significant bits, ties to even: fp32 rounding of t * 2^-34 in integer arithmetic"""
    t = np.asarray(t, np.int64)
    n = np.abs(t)
    assert (n < 2 ** 53).all()
    bl = np.frexp(n.astype(F64))[1].astype(np.int64)   # the bit length (n < 2^53: the conversion is exact)
    sh = np.maximum(bl - 24, 0)
    q, rem, half = n >> sh, n & ((np.int64(1) << sh) - 1), (np.int64(1) << sh) >> 1
    q = q + ((rem > half) | ((rem == half) & (sh > 0) & ((q & 1) == 1)))
    return np.sign(t) * (q << sh)


SCALE17, SCALE34 = 2.0 ** 17, 2.0 ** 34


def _exact_fma_sum(a, b):
    """P2._fma_sum's order with every fused multiply-add done in int64: operands are integers times 2^-17, partial sums times 2^-34"""
    (A, real), (Bv, _) = P2._entry_order(np.asarray(a, F32)), P2._entry_order(np.asarray(b, F32))
    Ai, Bi = A.astype(F64) * SCALE17, Bv.astype(F64) * SCALE17
    assert (Ai == np.round(Ai)).all() and (Bi == np.round(Bi)).all(), "an operand is no multiple of 2^-17"
    Ai, Bi = Ai.astype(np.int64), Bi.astype(np.int64)
    part = np.zeros((A.shape[0], NT), np.int64)
    for l in range(A.shape[1]):
        part = np.where(real[l][None, :], _round24(Ai[:, l] * Bi[:, l] + part), part)
    h = NT // 2
    while h >= 1:
        part = _round24(part[:, :h] + part[:, h:2 * h])
        h //= 2
    return (part[:, 0].astype(F64) / SCALE34).astype(F32)


def _f32_of_fraction(q):
    """a rational -> the nearest fp32 (normal range), ties to even, with no floating point on the way"""
    if q == 0:
        return F32(0)
    s, q = (-1 if q < 0 else 1), abs(q)
    e = 0
    while q >= 2 ** 24:
        q, e = q / 2, e + 1
    while q < 2 ** 23:
        q, e = q * 2, e - 1
    n, r = divmod(q.numerator, q.denominator)
    r = Fraction(r, q.denominator)
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2):
        n += 1
    return F32(s * float(n) * 2.0 ** e)   # n <= 2^24 and a power of two: exact


def _fraction_fma_sum(a, b):
    """one row [C, PP] each: the stated order with every fma an exact rational rounded once"""
    (A, real), (Bv, _) = P2._entry_order(np.asarray(a, F32)[None]), P2._entry_order(np.asarray(b, F32)[None])
    part = [F32(0)] * NT
    for l in range(A.shape[1]):
        for t in range(NT):
            if real[l, t]:
                part[t] = _f32_of_fraction(Fraction(float(A[0, l, t])) * Fraction(float(Bv[0, l, t])) + Fraction(float(part[t])))
    h = NT // 2
    while h >= 1:
        part = [_f32_of_fraction(Fraction(float(part[t])) + Fraction(float(part[t + h]))) for t in range(h)]
        h //= 2
    return part[0]


def _plain_sum(a, b):
    """P2._fma_sum's order with a plain multiply and a plain add in place of the fma (two roundings)"""
    (A, real), (Bv, _) = P2._entry_order(np.asarray(a, F32)), P2._entry_order(np.asarray(b, F32))
    part = np.zeros((A.shape[0], NT), F32)
    for l in range(A.shape[1]):
        part = np.where(real[l][None, :], ((A[:, l] * Bv[:, l]).astype(F32) + part).astype(F32), part)
    h = NT // 2
    while h >= 1:
        part = (part[:, :h] + part[:, h:2 * h]).astype(F32)
        h //= 2
    return part[:, 0]


@pytest.mark.parametrize("tier", Q.BIT_TIERS)
@pytest.mark.parametrize("case", Q.NORM_CASES, ids=CASE_IDS)
def test_fma_emulation_is_the_fma_on_the_bit_exact_sets(case, tier):
    x, y, g = Q.norm_inputs(case, tier)
    nbits, lo, hi = (12, 2.0 ** -6, 2.0 ** 3) if tier == "bits" else (16, 2.0 ** -2, 2.0 ** 2)
    for a in (x, y, g):
        nz = a[a != 0]
        assert (np.abs(nz) >= lo).all() and (np.abs(nz) < hi).all() and ((a == 0).any() or a.size < 8)
        m = np.frexp(a.astype(F64))[0] * 2.0 ** nbits
        assert (m == np.round(m)).all(), "more than %d significant bits" % nbits
    for a, b in ((x, x), (y, g)):
        got = P2._fma_sum(a, b)
        assert np.array_equal(R.bits(got), R.bits(_exact_fma_sum(a, b)))
        for r in (range(len(a)) if a.size <= 4000 else ()):   # the rational fma, independent of the integer one, on the small cases
            assert R.bits(F32(got[r])) == R.bits(_fraction_fma_sum(a[r], b[r])), r
        if tier == "bits":   # 24-bit products are fp32 values: without the fma the same bits — this set cannot see a missing fma
            assert np.array_equal(R.bits(got), R.bits(_plain_sum(a, b)))
    if tier == "bits16" and P2.norm_entries(case[0], case[1]) > 1000:   # ... the 16-bit set can, once a thread owns several entries
        assert not np.array_equal(R.bits(P2._fma_sum(y, g)), R.bits(_plain_sum(y, g)))
        assert not np.array_equal(R.bits(P2.normalize_backward_f32(x, y, g, Q.norm_mul(case))),
                                  R.bits(P2.normalize_backward_tail(_plain_sum(x, x), _plain_sum(y, g), y, g, Q.norm_mul(case))))
    C, PP, B, Mp = case
    if B >= 2:
        assert not x[B - 1].any() and not y[B - 1].any()
        s = F32(Q.norm_mul(case)) / np.sqrt(F32(1e-10))
        ref = P2.normalize_backward_f32(x, y, g, Q.norm_mul(case))
        assert np.isfinite(ref).all() and np.array_equal(R.bits(ref[B - 1]), R.bits((F32(s) * g[B - 1]).astype(F32)))
    if B >= 3:
        assert not g[0].any() and not P2.normalize_backward_f32(x, y, g, Q.norm_mul(case))[0].any()


def test_fma_emulation_differs_from_the_fma_at_full_mantissa():
    """one step of _fma_sum on full-mantissa operands the kernel could meet (factors near 2^-6, a partial sum near 2^12): the exact
    x * y + p lies 2^-58 below the tie between two fp32 values, float64 rounds it ONTO the tie, and ties-to-even then goes the other way"""
    x, y = F32(2.0 ** -6 * (1 + 2.0 ** -23)), F32(2.0 ** -6 * (1 - 2.0 ** -23))
    p = F32(4096.0 + 2.0 ** -11)   # an odd last bit: the tie rounds up
    emulated = F32(F64(x) * F64(y) + F64(p))
    exact = _f32_of_fraction(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(p)))
    assert exact == p and emulated == F32(4096.0 + 2.0 ** -10)
    assert R.bits(emulated) != R.bits(exact)


# ---- the tiers' conditions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", Q.NORM_CASES, ids=CASE_IDS)
def test_normalize_input_sets(case):
    C, PP, B, Mp = case
    mul = Q.norm_mul(case)
    # exact tier: both sums are integers below 2^24 in any order, and the stated order gives the same bits as the float64 sums
    x, y, g = Q.norm_inputs(case, "exact")
    assert (np.abs(x.astype(F64) * x).sum((1, 2)) < 2.0 ** 24).all() and (np.abs(y.astype(F64) * g).sum((1, 2)) < 2.0 ** 24).all()
    assert np.array_equal(R.bits(Q.normalize_backward_exact(x, y, g, mul)), R.bits(P2.normalize_backward_f32(x, y, g, mul)))
    # derived tier: the fp32 evaluation in the stated order meets the bound on the reference alone
    x, y, g = Q.norm_inputs(case, "derived")
    err = np.abs(P2.normalize_backward_f32(x, y, g, mul).astype(F64) - P2.normalize_backward64(x, y, g, mul))
    bound = P2.normalize_backward_bound(x, y, g, mul)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("ACC-CPU normalize_backward %s stated order err / bound = %.3f" % (case, ratio))
    assert (err <= bound).all(), ratio
    assert (bound <= 256 * 2.0 ** -24 * np.abs(P2.normalize_backward64(x, y, g, mul)).max()).all(), "the bound is slack"


def test_normalize_cases_cover_the_edges():
    E = {c: P2.norm_entries(c[0], c[1]) for c in Q.NORM_CASES}
    assert min(E.values()) == 8 and 256 in E.values() and any(e < 256 for e in E.values())
    assert E[(33, 8, 2, 4)] == 320 and (33 % 8, 9 % 8, 12 % 8, 3 % 8) == (1, 1, 4, 3)
    assert any(c[3] > c[2] for c in Q.NORM_CASES) and -(-E[(512, 49, 2, 2)] // NT) == 98
    assert sorted(Q.NORM_MUL.values()) == [0.37, 4.0] and all(k in Q.NORM_CASES for k in Q.NORM_MUL)


# ---- the gather ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("case", Q.GATHER_CASES, ids=["C%d_%dx%d_p%dx%d_N%d" % c for c in Q.GATHER_CASES])
def test_gather_chain_on_a_zeroed_map_is_the_ordered_sum(case, rule):
    C, H, W, PH, PW, N = case
    feat, rois, g, am = Q.gather_inputs(case, rule)
    zero = np.zeros((C, H, W), F32)
    for n0, n1 in K.roi_row_ranges(N):
        ref = K.roi_backward(g, am, rois, False, n0, n1, 1, C, H, W, F32)[0]
        assert np.array_equal(R.bits(Q.gather_chain(zero, g, am, n0, n1, W)), R.bits(ref))
        win = Q.gather_chain(zero, g, am, n0, n1, W, rois, PH, PW, K.ROI_SCALE, rule, windows=True)
        assert np.array_equal(R.bits(win), R.bits(ref)), "the forward's argmax lies in its window: the windowed chain is the plain one"
    # from a map that holds something: the chain continues, untouched cells keep their bits
    m0, special = Q.start_map(case, [am])
    out = Q.gather_chain(m0, g, am, 0, N, W)
    free = Q.untouched_cells([am], C, H, W).reshape(C, H, W)
    assert np.array_equal(R.bits(out[free]), R.bits(m0[free]))
    if free.sum() >= 2:
        assert len(special) == 2 and R.bits(out.reshape(C, -1)[special[0]]) == 0x80000000 and R.bits(out.reshape(C, -1)[special[1]]) == 0x7FC12345
    if H * W > 1:
        assert (R.bits(out[~free]) != R.bits(m0[~free])).any()
    err = np.abs(out.astype(F64) - Q.gather_chain(m0, g, am, 0, N, W, dtype=F64))
    bound = Q.gather_bound(m0, g, am, 0, N, W)
    ok = np.isfinite(err)
    assert (err[ok] <= bound[ok]).all() and (~ok).sum() <= 1


def test_gather_cases_hold_the_edges():
    """over the cases: an empty bin (argmax -1), a cell fed by two rows, a cell fed by nothing"""
    empty = two_rows = nothing = 0
    for case in Q.GATHER_CASES:
        C, H, W, PH, PW, N = case
        for rule in (0, 1):
            am = Q.gather_inputs(case, rule)[3]
            empty += int((am < 0).any())
            nothing += int(Q.untouched_cells([am], C, H, W).any())
            rows = np.zeros((C, H * W), np.int64)
            for n in range(N):
                rows += ~Q.untouched_cells([am[n:n + 1]], C, H, W)
            two_rows += int((rows >= 2).any())
    n = len(Q.GATHER_CASES)   # rule 0 leaves empty bins in every case (rule 1 clips the box first: none); the 1 x 1 map has no unfed cell
    assert empty == n and two_rows == 2 * n and nothing == 2 * (n - 1)
    assert {c[3:5] for c in Q.GATHER_CASES} == {(7, 7), (1, 1), (3, 5), (32, 32)} and any(c[0] % 8 for c in Q.GATHER_CASES)


@pytest.mark.parametrize("PH,PW,C,B", K.ROI_SYNTH_CASES)
def test_gather_synthetic_sequential_fp32_meets_its_bound(PH, PW, C, B):
    H, W, N = K.ROI_SYNTH_MAP
    am, g, _ = K.roi_synth_inputs(PH, PW, C, B)
    m0 = R.draw(np.random.default_rng([PH, PW, C, 53]), (C, H, W))
    err = np.abs(Q.gather_chain(m0, g, am, 0, N, W).astype(F64) - Q.gather_chain(m0, g, am, 0, N, W, dtype=F64))
    bound = Q.gather_bound(m0, g, am, 0, N, W)
    print("ACC-CPU gather synthetic p%dx%d C%d sequential err / bound = %.3f" % (PH, PW, C, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all() and err.max() > 0


# ---- int_to_float and the prefix launch ----------------------------------------------------------------------------------------------
def test_int_to_float_inputs():
    for n in Q.I2F_N:
        vs = Q.i2f_inputs(n)
        assert all(v.dtype == np.int32 and v.shape == (n,) for v in vs)
        seen = set(int(x) for v in vs for x in v)
        assert seen >= set(Q.I2F_SPECIAL)
        if n > 1:
            assert set(int(x) for x in vs[0][-7:]) == set(Q.I2F_SPECIAL)
    assert F32(np.int32(2 ** 24 + 1)) == F32(2 ** 24) and F32(np.int32(2 ** 31 - 1)) == F32(2.0 ** 31)   # round to nearest, ties to even
    assert np.array([2 ** 24 + 3], np.int32).astype(F32)[0] == F32(2 ** 24 + 4)


@pytest.mark.parametrize("N,PP,B", Q.DG_CASES)
def test_dgrad_prefix_inputs(N, PP, B):
    g, w, valid = Q.dgrad_inputs(N, PP, B)
    assert valid.sum() == PP * B and valid[:(PP - 1) * Q.DG_MP + B][-1] and (PP * Q.DG_MP == (PP - 1) * Q.DG_MP + B) == (B == Q.DG_MP)
    assert (np.abs(g.astype(F64)) @ np.abs(w.astype(F64))).max() < 2.0 ** 24   # every partial sum of any order is exact
    full, own = R.lin_pack(w, 1), R.lin_pack(w[:, :Q.DG_K], 1)
    assert full.shape[0] == 16 and own.shape[0] == 8
    assert np.array_equal(full[:Q.DG_K // 8], own[:Q.DG_K // 8]), "chunks < K / 8 of the wider pack are the K-column pack's"
    p44 = Q.lin_pack_zero_pad(w[:, :44])
    assert (R.bits(p44[5, :N, 4:]) == 0).all() and np.array_equal(p44[5, :N, :4], w[:, 40:44]) and np.isnan(p44[:, N:]).all()
    assert not np.array_equal(full[5, :N, 4:], p44[5, :N, 4:]), "in the wider pack lanes 44..47 hold the next slab's columns, not zeros"
