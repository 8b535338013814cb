"""The references of tests/test_gpu_graph_pool_numerics.py (tests/graph_pool_np.py) against the CPU oracle and PyTorch, over the shape
lists the GPU tests run: a wrong reference cannot pass here, so a kernel cannot pass against it there.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_pool_np as R  # noqa: E402

RNG = lambda seed: np.random.default_rng(seed)


@pytest.mark.parametrize("k,s,p,ceil", R.MAXPOOL_GEOMS)
def test_maxpool_matches_oracle_and_torch(O, k, s, p, ceil):
    n = 0
    for (H, W) in R.MAXPOOL_MAPS + [(5, 5)]:
        if pool_invalid(H, W, k, s, p, ceil):
            continue
        x = R.mixed_sign(RNG(H * 100 + W), (3, 5, H, W))
        y = R.maxpool64(x, k, s, p, ceil)
        assert y.shape[2:] == (O.pool_out_size(H, k, s, p, ceil), O.pool_out_size(W, k, s, p, ceil))
        np.testing.assert_array_equal(y, O.maxpool2d_mode(x, k, s, p, ceil).astype(np.float64))
        if 2 * p <= k:  # (PyTorch refuses pad > k / 2)
            t = F.max_pool2d(torch.from_numpy(x).double(), k, s, p, ceil_mode=bool(ceil)).numpy()
            np.testing.assert_array_equal(y, t)
        n += 1
    assert n >= 3


def pool_invalid(H, W, k, s, p, ceil):
    return min(R.pool_out_size(H, k, s, p, ceil), R.pool_out_size(W, k, s, p, ceil)) <= 0


def test_maxpool_minus_one_rule_fires():
    # (2, 2, 1, ceil) at H = 5: ceil((5 + 2 - 2) / 2) + 1 = 4 windows, but the 4th would start at 3 * 2 = 6 >= H + pad = 6: 3 outputs
    assert R.pool_out_size(5, 2, 2, 1, 1) == 3
    assert R.pool_out_size(5, 2, 2, 1, 0) == 3
    assert R.pool_out_size(5, 3, 2, 1, 1) == 3 and R.pool_out_size(6, 3, 2, 1, 1) == 4 and R.pool_out_size(6, 3, 2, 1, 0) == 3


def test_maxpool_edge_values():
    x = np.zeros((1, 1, 4, 4), np.float32)
    x[0, 0, :2, :2] = np.nan                      # an all-NaN window
    x[0, 0, 0, 2:] = [np.nan, -np.inf]
    x[0, 0, 1, 2:] = [-3.0, np.nan]
    x[0, 0, 2] = [np.inf, 1.0, -0.0, 0.0]
    y = R.maxpool64(x, 2, 2, 0, 0)[0, 0]
    assert y[0, 0] == -np.inf and y[0, 1] == -3.0 and y[1, 0] == np.inf and y[1, 1] == 0.0
    # padded cells never win: an all-negative map keeps its negative maxima on the border
    y = R.maxpool64(np.full((1, 1, 3, 3), -2.0, np.float32), 3, 2, 1, 1)
    assert (y == -2.0).all()


@pytest.mark.parametrize("geom", R.AVGPOOL_GEOMS)
def test_avgpool_matches_oracle_and_torch(O, geom):
    kh, kw, sh, sw, ph, pw = geom
    n = 0
    for (H, W) in R.AVGPOOL_MAPS:
        if H + 2 * ph < kh or W + 2 * pw < kw:
            continue
        x = R.mixed_sign(RNG(H * 100 + W), (2, 9, H, W))
        y = R.avgpool64(x, *geom)
        t = F.avg_pool2d(torch.from_numpy(x).double(), (kh, kw), (sh, sw), (ph, pw), count_include_pad=True).numpy()
        np.testing.assert_allclose(y, t, rtol=1e-13, atol=1e-13)
        seq = R.avgpool_seq32(x, *geom)
        cells = R.avgpool_cells(H, W, *geom)
        assert cells.shape == y.shape[2:] and cells.max() <= kh * kw and cells.min() >= 1
        bound = (cells + 2) * 2.0 ** -24 * R.avgpool64(np.abs(x), *geom)
        assert (np.abs(seq - y) <= bound).all()
        if kh == kw and sh == sw and ph == pw:  # the oracle's chain is the same order: bit-equal
            np.testing.assert_array_equal(seq, O.avgpool2d(x, kh, sh, ph))
        n += 1
    assert n >= 4


def test_avgpool_divisor_stays_full_window():
    for hw in (1, 2):
        x = np.ones((1, 1, hw, hw), np.float32)
        assert np.allclose(R.avgpool64(x, 3, 3, 1, 1, 1, 1), hw * hw / 9.0)
        assert (R.avgpool_seq32(x, 3, 3, 1, 1, 1, 1) == np.float32(hw * hw) * (np.float32(1) / np.float32(9))).all()
    b = np.array([-1.0], np.float32)
    assert (R.avgpool64(np.ones((1, 1, 1, 1)), 3, 3, 1, 1, 1, 1, bias=b, relu=True) == 0).all()
    assert np.allclose(R.avgpool64(np.ones((1, 1, 1, 1)), 3, 3, 1, 1, 1, 1, bias=b, relu=False), 1 / 9.0 - 1)


@pytest.mark.parametrize("size", R.LRN_SIZES)
@pytest.mark.parametrize("C", R.LRN_CHANNELS)
def test_lrn_matches_oracle_and_torch(O, C, size):
    for (alpha, beta, k) in R.LRN_PARAMS:
        x = R.mixed_sign(RNG(C * 31 + size), (1, C, 3, 5), -3, 7)
        y = R.lrn64(x, size, alpha, beta, k)
        t = F.local_response_norm(torch.from_numpy(x).double(), size, alpha, beta, k).numpy()
        np.testing.assert_allclose(y, t, rtol=1e-12)
        o = O.lrn(x, size, alpha, beta, k).astype(np.float64)
        assert (np.abs(o - y) <= 8 * 2.0 ** -24 * np.abs(y)).all()


@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("PH", R.ROI_POOLED)
def test_roi_pool_matches_oracle(O, PH, rule):
    for (H, W) in R.ROI_MAPS:
        rng = RNG(PH * 1000 + H * 10 + rule)
        feat = R.mixed_sign(rng, (3, H, W))
        for scale in (0.0625, 0.37):
            rois = R.roi_table(rng, 24, H, W, scale)
            y = R.roi_pool64(feat, rois, PH, PH, scale, rule)
            o = O.roi_pool(feat, rois, PH, PH, scale, bin_rule=rule)[0]
            np.testing.assert_array_equal(y, o.astype(np.float64))


def test_roi_table_covers_the_cases():
    H, W, scale = 38, 63, 0.0625
    rois = R.roi_table(RNG(1), 11, H, W, scale)
    empties = [sum(1 for a, b in R.roi_bins(r, scale, H, W, 7, 7, 0)[1] if b <= a) for r in rois]
    assert empties[0] == 0 and 0 < empties[1] < 7 and 0 < empties[2] < 7 and empties[5] == 7   # inside, across, wholly outside
    assert rois[7, 3] < rois[7, 1] and rois[8, 1] == rois[8, 3]                                # inverted, one pixel
    assert all(b > a for r in rois for a, b in R.roi_bins(r, scale, H, W, 7, 7, 1)[0])          # the adaptive rule: never empty


@pytest.mark.parametrize("PH,k,s,p", R.ROIMAX_GEOMS)
def test_roi_pool_then_maxpool(O, PH, k, s, p):
    for (H, W) in R.ROIMAX_MAPS:
        rng = RNG(PH + H)
        feat = -np.abs(R.mixed_sign(rng, (2, H, W)))   # all negative: an empty bin's 0 must win
        rois = R.roi_table(rng, 11, H, W, 0.0625)
        y = R.roi_pool_maxpool64(feat, rois, PH, 0.0625, 0, k, s, p)
        o = O.maxpool2d_mode(O.roi_pool(feat, rois, PH, PH, 0.0625, bin_rule=0)[0], k, s, p, 0)
        np.testing.assert_array_equal(y, o.astype(np.float64))
        assert (y[5] == 0).all() and (y < 0).any()
        if (H, W) == (38, 63):
            assert (y[0] < 0).all() and (y[1] == 0).any() and (y[1] < 0).any()


def test_global_average(O):
    for hw in (1, 6, 7, 8):
        x = R.mixed_sign(RNG(hw), (5, 9, hw, hw))
        seq = R.global_avg_seq32(x)
        np.testing.assert_array_equal(seq, O.avgpool_global(x))
        y = R.global_avg64(x)
        bound = (hw * hw + 2) * 2.0 ** -24 * np.abs(x).astype(np.float64).mean(axis=(2, 3))
        assert (np.abs(seq - y) <= bound).all()
        np.testing.assert_allclose(y, F.adaptive_avg_pool2d(torch.from_numpy(x).double(), 1).numpy()[:, :, 0, 0], rtol=1e-13)


def test_value_class_and_bf16_round():
    a = np.array([1.0, np.inf, -np.inf, np.nan, -0.0], np.float32)
    assert list(R.value_class(a)) == [0, 1, 2, 3, 0]
    assert R.bf16_round(np.array([1.00390625], np.float32))[0] == 1.0          # tie to even
    assert R.bf16_round(np.array([1.01171875], np.float32))[0] == 1.015625     # tie to even, upwards
