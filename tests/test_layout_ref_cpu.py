"""tests/layout_np.py checked without a GPU: every restatement against an independent formulation (torch permute / reshape / F.pad for the
layouts, F.max_pool2d(ceil_mode=True), F.unfold, torch's own bfloat16 conversion, float64 torch arithmetic for the image transformer),
pack -> unpack round trips, shard_owner against shard_bounds, and the halo record count — on the shape lists tests/test_gpu_layout_kernels.py
runs."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layout_np as L  # noqa: E402

F32 = np.float32


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _pad_dim(t, dim, to):
    pad = [0, 0] * (t.dim() - 1 - dim) + [0, to - t.shape[dim]]
    return Fn.pad(t, pad)


@pytest.mark.parametrize("H,W", L.MAP_HW)
@pytest.mark.parametrize("C", L.MAP_C)
def test_c8p(C, H, W):
    x = L.values([C, H, W], (C, H, W))
    Cb, Hp, Wp = L.cdiv(C, 8), L.act_hp(H), L.act_wp(W)
    t = _pad_dim(_t(x), 0, Cb * 8).reshape(Cb, 8, H, W).permute(0, 2, 3, 1)
    t = Fn.pad(t, (0, 0, 1, Wp - W - 1, 1, Hp - H - 1))
    assert _same(L.c8p_pack(x), t.numpy())
    assert _same(L.c8p_unpack(L.c8p_pack(x, pad=L.SENT_F, halo=L.SENT_F, pitch=L.SENT_F), C, H, W), x)
    real, pad, outside = L.c8p_masks(C, H, W)
    assert real.sum() == C * H * W and (real | pad | outside).all() and not (real & pad).any() and not (outside & (real | pad)).any()
    assert np.array_equal(outside, L.halo_mask(C, H, W))
    assert outside[0, :, :, 0].sum() == L.halo_records(H, W) == Hp * Wp - H * W


@pytest.mark.parametrize("M", L.ROWMAJOR_M)
@pytest.mark.parametrize("K", L.ROWMAJOR_K)
def test_c8(M, K):
    x = L.values([M, K], (M, K))
    Mp, q = L.lin_mp(M), L.cdiv(K, 8)
    t = _pad_dim(_pad_dim(_t(x), 1, q * 8), 0, Mp).reshape(Mp, q, 8).permute(1, 0, 2)
    assert _same(L.c8_pack(x, Mp), t.numpy())
    assert _same(L.c8_unpack(L.c8_pack(x, Mp, lane_fill=L.SENT_F, row_fill=L.SENT_F), M, K), x)


@pytest.mark.parametrize("N,C,PP,Mp", [(1, 1, 1, 1), (3, 9, 4, 5), (5, 17, 49, 128)])
def test_pooled(N, C, PP, Mp):
    x = L.values([N, C, PP], (N, C, PP))
    Cb = L.cdiv(C, 8)
    t = _pad_dim(_t(x), 1, Cb * 8).reshape(N, Cb, 8, PP).permute(1, 3, 0, 2).reshape(Cb * PP, N, 8)
    assert _same(L.pooled_pack(x, Mp), _pad_dim(t, 1, Mp).numpy())
    assert _same(L.pooled_unpack(L.pooled_pack(x, Mp, fill=L.SENT_F), N, C, PP), x)


@pytest.mark.parametrize("Cout", L.CONV_COUT)
@pytest.mark.parametrize("Cin", L.CONV_CIN)
def test_conv_pack(Cin, Cout):
    w = L.values([Cin, Cout], (Cout, Cin, 3, 3))
    nch, CoutP = L.cdiv(Cin, 8), L.conv_coutp(Cout)
    t = _pad_dim(_pad_dim(_t(w).reshape(Cout, Cin, 9), 1, nch * 8), 0, CoutP).reshape(CoutP, nch, 8, 9).permute(1, 3, 0, 2)
    assert _same(L.conv_pack(w), t.numpy())
    assert _same(L.gconv_pack(w.reshape(Cout, Cin, 9)), t.permute(1, 0, 2, 3).numpy())


@pytest.mark.parametrize("Cout", L.CONV_COUT)
@pytest.mark.parametrize("Cin", L.FIRST_CIN)
def test_conv_first_pack(Cin, Cout):
    w = L.values([Cin, Cout, 1], (Cout, Cin, 3, 3))
    CoutP = L.conv_coutp(Cout)
    t = _pad_dim(_pad_dim(_t(w).reshape(Cout, Cin, 9), 1, 4), 0, CoutP).permute(2, 1, 0).reshape(36, CoutP)   # row = tap * 4 + cin
    assert _same(L.conv_first_pack(w), t.numpy())


@pytest.mark.parametrize("KK,Cin,Cout", itertools.product(L.GCONV_KK, L.GCONV_CIN, L.GCONV_COUT))
def test_gconv_pack_and_bf16(KK, Cin, Cout):
    w = L.values([KK, Cin, Cout], (Cout, Cin, KK))
    nch, CoutP = L.cdiv(Cin, 8), L.round_up(Cout, 128)
    nch2 = L.round_up(nch, 2)
    t = _pad_dim(_pad_dim(_t(w), 1, nch2 * 8), 0, CoutP).reshape(CoutP, nch2, 8, KK).permute(3, 1, 0, 2).contiguous()
    assert _same(L.gconv_pack(w), t[:, :nch].contiguous().numpy())
    assert _same(L.gconv_pack(w, nch=nch2), t.numpy())
    b = t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(L.f2bf_bits(L.gconv_pack(w, nch=nch2)), b)


def test_f2bf_ties_and_edges():
    u = np.array([0x3F800000, 0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0x00000001, 0x00008000, 0x00018000,
                  0x80000000, 0x7F7F8000, 0x7F7F7FFF], np.uint32)
    want = np.array([0x3F80, 0x3F80, 0x3F82, 0x3F81, 0x3F80, 0x7F80, 0xFF80, 0x7F80, 0x0000, 0x0000, 0x0002, 0x8000, 0x7F80, 0x7F7F], np.uint16)
    assert np.array_equal(L.f2bf_bits(u.view(F32)), want)
    assert np.array_equal(_t(u.view(np.int32)).view(torch.float32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16), want)


@pytest.mark.parametrize("Cout,KK", itertools.product(L.PERMUTE_COUT, L.PERMUTE_KK))
def test_permute_w3(Cout, KK):
    w = L.values([Cout, KK], (Cout, 3, KK))
    assert _same(L.permute_w3(w), _t(w).permute(0, 2, 1).reshape(Cout, KK * 3).numpy())


@pytest.mark.parametrize("H,W", L.MAP_HW)
@pytest.mark.parametrize("swap,scale,has_std", itertools.product(L.IMAGE_SWAPS, L.IMAGE_SCALES, (0, 1)))
def test_image_transform(H, W, swap, scale, has_std):
    img, mean = L.image_case(H, W, swap, scale, 0)
    got = L.image_transform(img, swap, scale, mean, L.IMAGE_STD, has_std)
    t = _t(img)[list(swap)].double()
    if scale != 1.0:
        t = t * scale
    t = t - torch.tensor(mean, dtype=torch.float64)[:, None, None]
    if has_std:
        t = t / torch.tensor(L.IMAGE_STD, dtype=torch.float64)[:, None, None]
    assert _same(got, t.float().numpy())
    # the special pixels are what image_case says they are
    d = [1.0 / s if has_std else 1.0 for s in L.IMAGE_STD]
    assert got[0, 0, 0] == F32(2.0 ** -140 * d[0]) and 0 < got[0, 0, 0] < np.finfo(F32).tiny
    assert got[1, 0, 0] == F32((1.0 + 2.0 ** -22) * d[1])                      # the tie went up, to the even neighbour
    if W > 1:
        k = 255 if scale != 1.0 else 1
        assert got[1, 0, 1] == F32((1.0 + (1 + k) * 2.0 ** -23) * d[1])        # the tie went down, to the even neighbour
    for Hc, Wc in ((H + a, W + b) for a, b in L.CANVAS_EXTRA):
        m = L.image_c8p(got, Hc, Wc, outside=L.SENT_F)
        canvas = Fn.pad(_pad_dim(_t(got), 0, 8), (0, Wc - W, 0, Hc - H))
        assert _same(L.c8p_unpack(m, 8, Hc, Wc), canvas.numpy())
        assert (L.bits(m[L.halo_mask(3, Hc, Wc)]) == L.SENT).all()


@pytest.mark.parametrize("H,W", L.POOL_HW)
@pytest.mark.parametrize("C", L.POOL_C)
def test_maxpool2x2(C, H, W):
    x = np.where(np.isfinite(L.pool_input(C, H, W, 0)), L.pool_input(C, H, W, 0), F32(1.5))   # torch's pool propagates NaN: NaN-free here
    x = np.where(x == 0, F32(0.0), x).astype(F32)                                             # (and one sign of zero)
    assert _same(L.maxpool2x2(x), Fn.max_pool2d(_t(x)[None], 2, 2, ceil_mode=True)[0].numpy())
    y = L.maxpool2x2(L.pool_input(C, H, W, 0))
    assert not np.isnan(y).any()
    if H >= 2 and W >= 2:
        assert np.isneginf(y[C - 1, 0, 0])                                   # the all-NaN window
        assert L.bits(y[0, 0, 0]) == 0x80000000                              # -0.0 met first, +0.0 is not greater
    if H >= 3 and W >= 4:
        assert L.bits(y[0, 0, 1]) == 0 and np.isneginf(y[0, 1, 0])           # +0.0 met first; -inf and NaN only


@pytest.mark.parametrize("n", L.HALO_N)
def test_halo_list_mixes_geometries(n):
    lst = L.halo_list(n)
    assert len(lst) == n and (n < 2 or len(set(lst)) > 1)
    for C, H, W in lst:
        assert C in L.HALO_C and (H, W) in L.HALO_HW
    if n >= len(L.HALO_C) * len(L.HALO_HW):
        assert len(set(lst)) == len(L.HALO_C) * len(L.HALO_HW)


def test_shard_owner_inverts_shard_bounds():
    for n in range(0, 41):
        for world in range(1, 10):
            seen = 0
            for rank in range(world):
                lo, hi = L.shard_bounds(n, world, rank)
                assert lo == seen and 0 <= hi - lo <= L.cdiv(n, world) if n else hi == lo == 0
                for item in range(lo, hi):
                    assert L.shard_owner(item, n, world) == (rank, item - lo)
                seen = hi
            assert seen == n


@pytest.mark.parametrize("N,world,P,C", L.SHARD_ROWS)
def test_shard_rows(N, world, P, C):
    sc, bb = L.values([N, world, P, C], (P, N, C)), L.values([N, world, P, C, 1], (P, N, 4 * C))
    recs = []
    for rank in range(world):
        lo, hi = L.shard_bounds(N, world, rank)
        recs.append(L.shard_rows_record(sc[:, lo:hi], bb[:, lo:hi], N, world, rank, P, C))
        assert recs[-1].size == P * L.cdiv(N, world) * 5 * C
    s2, b2 = L.shard_rows_join(np.stack(recs), N, world, P, C)
    assert _same(s2, sc) and _same(b2, bb)


@pytest.mark.parametrize("n_cls,world,rows", itertools.product(L.SHARD_CLS, L.SHARD_WORLD, (1, 64)))
def test_shard_classes_round_trip(n_cls, world, rows):
    rng = np.random.default_rng([n_cls, world, rows])
    keep, voted = L.values([n_cls, rows, 1], (n_cls, rows, 5)), L.values([n_cls, rows, 2], (n_cls, rows, 5))
    kidx = rng.integers(-2 ** 31, 2 ** 31, (n_cls, rows)).astype(np.int32)
    n_keep = rng.integers(-2, rows + 3, n_cls).astype(np.int32)
    for v in (None, voted):
        recs = np.stack([L.shard_class_record(keep, kidx, n_keep, v, n_cls, world, r, rows) for r in range(world)])
        k2, i2, n2, v2 = L.shard_class_join(recs, n_cls, world, rows, v is not None)
        assert np.array_equal(n2, np.clip(n_keep, 0, rows))
        for c in range(n_cls):
            n = n2[c]
            assert np.array_equal(k2[c, :n], L.bits(keep[c, :n])) and np.array_equal(i2[c, :n].view(np.int32), kidx[c, :n])
            assert (k2[c, n:] == L.SENT).all() and (i2[c, n:] == L.SENT).all()
            if v is not None:
                assert np.array_equal(v2[c, :n], L.bits(voted[c, :n])) and (v2[c, n:] == L.SENT).all()


@pytest.mark.parametrize("top_cap", L.DET_CAP)
def test_det_record(top_cap):
    dets = L.values([top_cap], (top_cap, 6))
    for n in (-3, 0, 1, top_cap, top_cap + 5):
        rec = L.det_record(dets, n, top_cap)
        c = min(max(n, 0), top_cap)
        assert rec[-1] == c and _same(rec[:c * 6], dets[:c].reshape(-1)) and (L.bits(rec[c * 6:-1]) == 0).all()


@pytest.mark.parametrize("H,W", L.MAP_HW)
@pytest.mark.parametrize("Cb", L.C8I_CB)
def test_c8i_and_pixel_major(Cb, H, W):
    C = Cb * 8
    x = L.values([Cb, H, W], (1, C, H, W))
    pitch = L.c8i_pitch(H * W)
    t = _pad_dim(_t(x)[0].reshape(Cb, 8, H * W).permute(0, 2, 1), 1, pitch)
    assert _same(L.c8i_pack(x), t.numpy())
    assert _same(L.c8i_unpack(L.c8i_pack(x, L.SENT_F, L.SENT_F), 1, C, H, W), x)
    assert _same(L.pixel_major(x[0]), _t(x)[0].permute(1, 2, 0).reshape(H * W, C).numpy())


@pytest.mark.parametrize("N,H,W,mx", L.MOSAIC)
def test_mosaic(N, H, W, mx):
    C, cap = 8, N + L.MOSAIC_SPARE
    x = L.values([N, H, W, mx], (N, C, H, W))
    rows, cols = L.mosaic_dims(cap, H, W, mx)
    # cells of (H + 1) x (W + 1), the map top-left: pad each map by one row and column behind, tile, then lay out as C8P
    cells = Fn.pad(_t(x), (0, 1, 0, 1))
    cells = _pad_dim(cells, 0, L.cdiv(cap, mx) * mx).reshape(L.cdiv(cap, mx), mx, C, H + 1, W + 1).permute(2, 0, 3, 1, 4).reshape(C, rows, cols)
    assert _same(L.mosaic_pack(x, cap, mx), L.c8p_pack(cells.numpy()))
    # separators, spare cells and halo are exactly the records no map pixel lands on
    m = L.mosaic_pack(np.ones_like(x), cap, mx, fill=0.0)
    assert m.sum() == N * C * H * W


@pytest.mark.parametrize("H,W", L.IM2COL_HW)
@pytest.mark.parametrize("KH,KW,stride,pad", L.IM2COL_K)
def test_im2col3(KH, KW, stride, pad, H, W):
    img = L.values([KH, stride, H, W], (3, H, W))
    img = np.where(np.isfinite(img), img, F32(2.5)).astype(F32)   # (unfold multiplies nothing, but keep the comparison NaN- and inf-free)
    got = L.im2col3(img, KH, KW, stride, pad, row_fill=L.SENT_F)
    u = Fn.unfold(_t(img)[None], (KH, KW), padding=pad, stride=stride)[0]     # [c * KK + tap, L]
    P, KK = u.shape[1], KH * KW
    ref = u.reshape(3, KK, P).permute(2, 1, 0).reshape(P, KK * 3)             # [pixel, tap * 3 + c]
    nkb = L.round_up(KK * 3, 64) // 8
    assert got.shape == (nkb, L.c8i_pitch(P), 8)
    assert _same(L.c8_unpack(got, P, KK * 3), ref.numpy())
    assert (L.bits(L.c8_unpack(got, P, nkb * 8)[:, KK * 3:]) == 0).all() and (L.bits(got[:, P:]) == L.SENT).all()
