"""tests/roi_pool_np.py on the CPU: its references against the CPU oracle's roi_pool (values and arg-max, both bin rules) and against
torch.nn.functional.normalize in float64, its two fp32 restatements of the normalisation inside their derived bounds on every input set
the GPU file runs, its layouts against each other, and the NaN example of the range-max tables pinned on the references."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roi_pool_np as R  # noqa: E402

F32, F64 = np.float32, np.float64
FINITE_CASES = [c for c in R.pool_cases() if c[4] != "edge"]


@pytest.mark.parametrize("case", FINITE_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_references_against_the_oracle(O, case):
    C, H, W, N, kind, rule, scale, Mp, stride, region, PH, PW = case
    feat, rois, ref = R.pool_inputs(C, H, W, N, kind, rule, scale, PH, PW)
    out, arg = O.roi_pool(feat, rois, PH, PW, scale, bin_rule=rule)
    assert np.array_equal(ref, out.astype(F64))
    assert np.array_equal(R.roi_argmax(feat, rois, PH, PW, scale, rule), arg)


def test_every_shape_is_covered():
    cases = R.pool_cases()
    for C, H, W in R.MAPS:
        for N in R.MAP_N[(C, H, W)]:
            for rule in (0, 1):
                assert any(c[:6] == (C, H, W, N, "edge", rule) for c in cases)
    assert {c[6] for c in cases} == set(R.SCALES) and {c[8] for c in cases} == {5, 20} and {c[9] for c in cases if c[8] == 20} == {0, 1, 2, 3}
    assert {(c[10], c[11]) for c in cases} == {(7, 7)} | set(R.OTHER_BINS)
    assert any(c[7] % 128 for c in cases) and any(c[7] == 0 for c in cases)
    assert R.vmax_levels(1) == 0 and R.vmax_levels(2) == 1 and R.vmax_levels(21) == 4 and R.vmax_levels(33) == 5
    assert R.cdiv(264, 8) == 33 and 49 * R.cdiv(33, 32) == 98  # the second 256-channel slice; G = 98 > 64


def test_layouts():
    rng = np.random.default_rng(5)
    C, H, W = 11, 5, 7
    x = rng.standard_normal((C, H, W)).astype(F32)
    m = R.c8p_pack(x)
    assert m.size == R.act_elems(C, H, W)
    flat = m.reshape(-1)
    Hp, Wp = R.act_hp(H), R.act_wp(W)
    for c, y, xx in ((0, 0, 0), (10, 4, 6), (7, 2, 3), (8, 0, 6)):
        assert flat[((c // 8 * Hp + y + 1) * Wp + xx + 1) * 8 + c % 8] == x[c, y, xx]
    u = R.c8p_unpack(m, C, H, W)
    assert np.array_equal(u[:C], x) and (R.bits(u[C:]) == 0).all()
    assert (m[:, 0] == R.HALO).all() and (m[:, :, 0] == R.HALO).all() and (m[:, H + 1:] == R.HALO).all() and (m[:, :, W + 1:] == R.HALO).all()
    pm = np.ascontiguousarray(u.transpose(1, 2, 0))
    assert pm.reshape(-1)[(3 * W + 2) * 16 + 9] == x[9, 3, 2] and np.array_equal(R.pm_unpack(pm, C, H, W), u)
    N, PP, Mp = 3, 6, 8
    p = rng.standard_normal((N, 16, PP)).astype(F32)
    c8 = R.c8_pack(p, Mp)
    for n, c, b in ((0, 0, 0), (2, 15, 5), (1, 8, 3)):
        assert c8.reshape(-1)[R.c8_index(c // 8, b, n, c % 8, PP, Mp)] == p[n, c, b]
    back = R.c8_unpack(c8, 16, PP, Mp)
    assert np.array_equal(back[:N], p) and (R.bits(back[N:]) == R.SENT).all()


def test_nan_examples_on_the_references():
    """a pooling window ignores its NaNs: [NaN, 5] over rows [0, 2) gives 5, [1, 3, NaN, 9] over rows [0, 4) gives 9.  A select that keeps a
    NaN left operand (b > a ? b : a) gives -inf and 3: emulated here beside the references."""
    for col, want, broken in (([np.nan, 5.0], 5.0, -np.inf), ([1.0, 3.0, np.nan, 9.0], 9.0, 3.0)):
        H = len(col)
        feat = np.array(col, F32).reshape(1, H, 1)
        rois = np.array([[1, 1, 1, 1, H]], F32)
        for rule in (0, 1):
            assert R.roi_bins(rois[0], 1.0, H, 1, 1, 1, rule) == ([(0, H)], [(0, 1)])
            assert R.roi_pool64(feat, rois, 1, 1, 1.0, rule)[0, 0, 0, 0] == want
            assert R.roi_argmax(feat, rois, 1, 1, 1.0, rule)[0, 0, 0, 0] == col.index(want)
        T = R.vmax_tables64(feat)
        k = R.vmax_levels(H)
        assert T[k, 0, 0, 0] == want

        def sel(a, b):  # the select the table builders and readers used
            return b if b > a else a
        lv = list(col)
        for step in [1 << i for i in range(k)]:
            lv = [sel(lv[y], lv[y + step]) if y + step < H else lv[y] for y in range(H)]
        v = sel(lv[0], lv[H - (1 << k)])
        m = v if v > -np.inf else -np.inf
        assert m == broken
    T = R.vmax_tables64(np.array([np.nan, np.nan, 1.0], F32).reshape(1, 3, 1))
    assert np.isnan(T[1, 0, 0, 0]) and T[1, 0, 1, 0] == 1.0 and T[1, 0, 2, 0] == 1.0


def test_l2norm64_against_torch():
    rng = np.random.default_rng(11)
    x = rng.standard_normal((7, 300))
    y, s = R.l2norm64(x, 1000.0)
    t = torch.nn.functional.normalize(torch.from_numpy(x), p=2, dim=1, eps=0.0).numpy() * 1000.0
    assert np.abs(y - t).max() <= 1e-9 * np.abs(t).max()  # (1e-10 under the root against |x|^2 ~ 300)
    assert np.allclose(s, 1000.0 / np.sqrt((x * x).sum(1) + 1e-10), rtol=1e-15)


def _inside(tag, got, ref, K, ops):
    bound = R.l2norm_bound(ref, K, ops)
    err = np.abs(np.asarray(got, F64) - ref)
    assert np.isfinite(err).all(), tag
    assert (err <= bound).all(), (tag, float((err / np.maximum(bound, 1e-300)).max()))
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


@pytest.mark.parametrize("case", R.norm_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_fp32_orders_inside_their_bounds_fused(case):
    C, H, W, N, kind, rule, scale, Mp, mul = case
    feat, rois, ref = R.pool_inputs(C, H, W, N, kind, rule, scale, 7, 7, True)
    p = R.pooled_padded(ref, C)
    y, s = R.l2norm_fused_f32(p, mul)
    if kind == "huge":
        live = (p != 0).any(axis=(1, 2))  # (the ROIs wholly outside pool zeros)
        assert live.any() and (y == 0).all() and (s[live] == 0).all()  # the sum of squares overflows: d = inf, v / d = 0, mul / d = 0
        return
    y64, s64 = R.l2norm64(p.reshape(N, -1), mul)
    K = p.shape[1] * p.shape[2]
    _inside("fused in place", y.reshape(N, -1), y64, K, 2)
    _inside("fused scale", s, s64, K, 1)
    c8 = R.l2norm_c8_f32(R.c8_pack(p, R.lin_mp(N)), N, mul)
    _inside("l2norm_scale_c8", R.c8_unpack(c8, C, 49, R.lin_mp(N))[:N].reshape(N, -1), y64, K, 2)
    if kind == "zero" or rule == 0:  # an all-zero ROI: zeros and a finite scale
        assert (R.bits(y[0]) == 0).all() and np.isfinite(s[0]) and s[0] == F32(mul) / np.sqrt(R.EPS32)


@pytest.mark.parametrize("nrec,N,Mp", R.L2_CASES)
def test_fp32_orders_inside_their_bounds_c8(nrec, N, Mp):
    x = R.l2_inputs(nrec, N, Mp)
    y = R.l2norm_c8_f32(x, N, 0.37)
    assert (R.bits(y[:, N:, :]) == R.SENT).all()
    v = x[:, :N, :].transpose(1, 0, 2).reshape(N, -1)
    y64, _ = R.l2norm64(v, 0.37)
    _inside("l2norm_scale_c8", y[:, :N, :].transpose(1, 0, 2).reshape(N, -1), y64, nrec * 8, 2)
