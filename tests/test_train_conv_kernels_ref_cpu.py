"""tests/train_conv_kernels_np.py checked on the CPU: the restatements agree with each other and with PyTorch-CPU
float64 autograd (conv2d backward, max-pool backward, a gather at a given arg-max), and — for every input set of
tests/test_gpu_train_conv_kernels_numerics.py — a plain sequential fp32 evaluation meets each derived bound, and every exact-tier input set
really is exact in float64 and below 2^24 in magnitude.  No GPU case may use inputs for which the reference alone would not pass.  The
largest CPU ratio per family is printed (CPU ...)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_conv_kernels_np as K  # noqa: E402
import train_conv_np as TC  # noqa: E402
import train_kernels_np as R  # noqa: E402
import train_trunk_np as TT  # noqa: E402

F32, F64 = np.float32, np.float64


def _same(a, b):
    return np.array_equal(R.bits(a), R.bits(b))


def _ratio(err, bound):
    nz = bound > 0
    assert np.isfinite(err).all() and (err[~nz] == 0).all()
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


# ---- layouts -----------------------------------------------------------------------------------------------------------------------------
def test_c8p_layout():
    x = R.draw(np.random.default_rng(1), (12, 9, 35), zero_frac=0.0)
    m = K.c8p_pack(x, pad=1.0, halo=2.0, pitch=3.0)
    assert m.shape == (2, 18, 66, 8) and _same(K.c8p_unpack(m, 12, 9, 35), x)
    assert m.reshape(-1)[((1 * 18 + 4 + 1) * 66 + 30 + 1) * 8 + 3] == x[11, 4, 30]   # dense.h's address rule
    real, pad, outside = K.c8p_masks(12, 9, 35)
    assert real.sum() == x.size and pad.sum() == 4 * 9 * 35 and (m[pad] == 1).all()
    assert set(np.unique(m[outside])) == {2.0, 3.0}
    assert (m[:, 0, :37] == 2).all() and (m[:, 10, :37] == 2).all() and (m[:, :11, 0] == 2).all() and (m[:, :11, 36] == 2).all()
    assert (m[:, 11:] == 3).all() and (m[:, :, 37:] == 3).all()
    assert _same(K.c8p_pack(x), R.c8p_pack(x))


@pytest.mark.parametrize("Cin,Cout", K.DGRAD_PACK_SHAPES)
def test_dgrad_weights_compute_the_input_gradient(Cin, Cout):
    rng = np.random.default_rng([Cin, Cout])
    w = rng.standard_normal((Cout, Cin, 3, 3))
    x = torch.tensor(rng.standard_normal((1, Cin, 4, 5)), requires_grad=True)
    g = torch.tensor(rng.standard_normal((1, Cout, 4, 5)))
    torch.nn.functional.conv2d(x, torch.tensor(w), padding=1).backward(g)
    dx = torch.nn.functional.conv2d(g, torch.tensor(K.dgrad_weights(w)), padding=1)
    assert np.allclose(dx.numpy(), x.grad.numpy(), rtol=1e-12, atol=1e-12)
    wpk_t, zb = K.dgrad_pack(w.astype(F32))
    assert wpk_t.shape == (K.cdiv(Cout, 8), 9, K.conv_coutp(Cin), 8) and zb.shape == (K.conv_coutp(Cin),)
    assert _same(K.conv_unpack(wpk_t, Cout, Cin), K.dgrad_weights(w.astype(F32)))
    assert (R.bits(wpk_t)[~K.conv_valid(Cout, Cin)] == 0).all()
    assert wpk_t[(Cout - 1) // 8, 2 * 3 + 0, Cin - 1, (Cout - 1) % 8] == F32(w[Cout - 1, Cin - 1, 0, 2])


# ---- ROI pooling backward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.ROI_CASES)
def test_roi_restatements(case):
    C, H, W, PH, PW, N, B = case
    feat, rois, g = K.roi_inputs(*case)
    nb = max(B, 1)
    # the half-integer corners are exact in fp32 and do sit on roundf's boundary
    p = (rois[1, 1:].astype(F32) - F32(1)) * F32(K.ROI_SCALE)
    assert (np.abs(p - np.floor(p)) == 0.5).all() and (rois[3, 1:] - 1 < 0).any() if N > 3 else True
    w0 = K.roi_windows(rois, H, W, PH, PW, K.ROI_SCALE, 0)
    ref = TC.roi_windows(rois, H, W, PH, PW, K.ROI_SCALE)
    for n in range(N):
        for ph in range(PH):
            for pw in range(PW):
                assert ref[n][ph * PW + pw] == (w0[0][n, ph], w0[1][n, ph], w0[2][n, pw], w0[3][n, pw])
    rows = K.roi_rows_map(rois, nb)
    for rule in (0, 1):
        hs, he, ws, we = K.roi_windows(rois, H, W, PH, PW, K.ROI_SCALE, rule)
        assert (hs >= 0).all() and (he <= H).all() and (ws >= 0).all() and (we <= W).all()
        if rule == 1:
            assert (he > hs).all() and (we > ws).all()   # never empty
        am = np.stack([K.window_argmax(feat[rows[n]], rois[n:n + 1], PH, PW, K.ROI_SCALE, rule)[0] for n in range(N)])
        assert K.argmax_in_windows(am, rois, H, W, PH, PW, K.ROI_SCALE, rule)
        if rule == 0:
            assert (am < 0).any()   # the box outside the map
            own = np.stack([TC.own_argmax(feat[rows[n]], rois[n:n + 1], PH, PW, K.ROI_SCALE)[0] for n in range(N)])
            assert np.array_equal(own, am)
        for n0, n1 in ([(0, N)] if B else K.roi_row_ranges(N)):
            got = K.roi_backward(g, am, rois, B > 0, n0, n1, nb, C, H, W, F32)
            sel = np.zeros(N, bool)
            sel[n0:n1] = True
            r5 = rois.copy()
            r5[:, 0] = rows + 1
            if n0 == n1:
                assert (R.bits(got) == 0).all()
                continue
            want = TC.roi_pool_backward_np(g[sel], am[sel], r5[sel], nb, C, H, W, np.float32)
            assert _same(got, want)
        # float64 against autograd: the pooling as a gather at the given arg-max
        got64 = K.roi_backward(g, am, rois, B > 0, 0, N, nb, C, H, W, F64)
        ft = torch.tensor(feat.astype(F64), requires_grad=True)
        for n in range(N):
            TC.gather_pool(ft[rows[n]], am[n:n + 1]).backward(torch.tensor(g[n:n + 1].astype(F64)))
        assert np.allclose(got64, ft.grad.numpy(), rtol=1e-12, atol=1e-12)
    # the C8 matrix of the trainer's layout
    c8 = K.roi_g_c8(g, 128, fill=R.SENT_F)
    assert c8.shape == (K.cdiv(C, 8) * PH * PW, 128, 8)
    n, c, b = N - 1, C - 1, PH * PW - 1
    assert c8.reshape(-1)[n * 8 + (c // 8) * (PH * PW * 128 * 8) + (c % 8) + b * 128 * 8] == g[n, c, b]   # train_conv_backward's strides
    assert (R.bits(c8) == R.SENT).sum() == c8.size - g.size


@pytest.mark.parametrize("PH,PW,C,B", K.ROI_SYNTH_CASES)
def test_roi_synthetic_sum_meets_its_bound(PH, PW, C, B):
    """the ordered fp32 sum is itself the sequential evaluation: |r - r64| <= (n + 1) * 2^-23 * sum |g| over the n terms of a cell"""
    H, W, N = K.ROI_SYNTH_MAP
    am, g, rois = K.roi_synth_inputs(PH, PW, C, B)
    run = lambda v, dt: K.roi_backward(v, am, rois, True, 0, N, B, C, H, W, dt)
    cnt = run(np.ones_like(g), F64)
    assert cnt.max() > 30   # heavy collisions
    _note("roi_pool_backward sum", _ratio(np.abs(run(g, F32).astype(F64) - run(g, F64)), (cnt + 1) * K.U23 * run(np.abs(g), F64)))


# ---- weight and bias gradients -----------------------------------------------------------------------------------------------------------
WORST = {}


def _note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print("CPU %-28s err / bound = %.3f (largest so far %.3f)" % (family, ratio, WORST[family]))
    assert ratio < 1.0, family


@pytest.mark.parametrize("shape", K.WGRAD_SHAPES)
def test_wgrad_reference_and_bounds(shape):
    Cin, Cout, H, W = shape
    for exact in (False, True):
        imgs = K.wgrad_inputs(*shape, exact=exact)
        tot64 = np.zeros((Cout, Cin, 3, 3))
        tot_mag = np.zeros_like(tot64)
        chain = np.zeros((Cout, Cin, 3, 3), F32)
        for i, (x, g) in enumerate(imgs):
            s64, mag, npx = K.wgrad_slabs64(x, g)
            assert len(npx) == K.n_segments(H, W) and sum(npx) == H * W and all(n == K.SEG_PX for n in npx[:-1])
            xt = torch.tensor(x.astype(F64)[None])
            wt = torch.zeros((Cout, Cin, 3, 3), dtype=torch.float64, requires_grad=True)
            torch.nn.functional.conv2d(xt, wt, padding=1).backward(torch.tensor(g.astype(F64)[None]))
            assert np.allclose(s64.sum(0), wt.grad.numpy(), rtol=1e-12, atol=1e-12)
            seq = K.wgrad_slabs_seq_f32(x, g)
            if exact:
                assert (mag.sum(0) < 2.0 ** 24).all() and (s64 == np.round(s64)).all()
                assert _same(seq, s64.astype(F32)) and _same(K.group_sum_f32(seq), s64.sum(0).astype(F32))
            else:
                assert (np.abs(x)[x != 0] >= 2.0 ** -6).all() and (np.abs(x) <= 8).all() and (np.abs(g) <= 8).all()
                for s in range(len(npx)):
                    _note("conv3x3_wgrad part", _ratio(np.abs(seq[s].astype(F64) - s64[s]), (npx[s] + 1) * K.U23 * mag[s]))
            for s in range(len(npx)):   # one chain over every pixel of every image
                chain = chain + seq[s] if exact else _chain(chain, x, g, s)
            tot64, tot_mag = tot64 + s64.sum(0), tot_mag + mag.sum(0)
            n = H * W * (i + 1) + (i + 1)
            if exact:
                assert (tot_mag < 2.0 ** 24).all() and _same(chain, tot64.astype(F32))
            else:
                _note("conv3x3_wgrad dw", _ratio(np.abs(chain.astype(F64) - tot64), (n + 1) * K.U23 * tot_mag))
        # the packing of the slabs and the emulated reduce are consistent with the plain sums
        x, g = imgs[0]
        seq = K.wgrad_slabs_seq_f32(x, g)
        part = K.slabs_pack(seq, fill=R.SENT_F)
        assert _same(K.slabs_unpack(part, Cin, Cout), seq)
        dw = K.wgrad_reduce_f32(part, Cin, Cout)
        assert _same(K.conv_unpack(dw, Cin, Cout), K.group_sum_f32(seq)) and (R.bits(dw)[~K.conv_valid(Cin, Cout)] == 0).all()
        old = K.conv_pack(R.draw(np.random.default_rng(3), (Cout, Cin, 3, 3)), fill=R.SENT_F)
        acc = K.wgrad_reduce_f32(part, Cin, Cout, old)
        assert _same(K.conv_unpack(acc, Cin, Cout), K.conv_unpack(old, Cin, Cout) + K.group_sum_f32(seq))
        assert (R.bits(acc)[~K.conv_valid(Cin, Cout)] == 0).all()


def _chain(acc, x, g, s):
    """continue ONE fp32 chain over the pixels of segment s of (x, g)"""
    P = K._patches(np.asarray(x, F32)).transpose(2, 1, 0)
    gf = np.asarray(g, F32).reshape(g.shape[0], -1).T
    for p in range(s * K.SEG_PX, min((s + 1) * K.SEG_PX, gf.shape[0])):
        acc = acc + (gf[p][:, None, None] * P[p][None]).reshape(acc.shape)
    return acc


def test_group_sum_order():
    rng = np.random.default_rng(5)
    for nseg in (1, 7, 8, 9, 17):
        s = R.draw(rng, (nseg, 64))
        plain = np.zeros(64, F32)
        for i in range(nseg):
            plain = plain + s[i]
        got = K.group_sum_f32(s)
        if nseg <= K.SEG_GROUP:
            assert _same(got, plain)
        else:
            groups = [K.group_sum_f32(s[i:i + 8]) for i in range(0, nseg, 8)]
            want = groups[0]
            for q in groups[1:]:
                want = want + q
            # 8 + 1 slabs is still the plain chain; from a second full group on the order differs (somewhere in 64 draws)
            assert _same(got, want) and _same(got, plain) == (nseg == 9)


@pytest.mark.parametrize("Cout,H,W", K.bias_maps())
def test_bias_grad_reference_and_bounds(Cout, H, W):
    for exact in (False, True):
        gs = K.bias_inputs(Cout, H, W, exact)
        seq, tot64, mag, db = np.zeros(Cout, F32), np.zeros(Cout), np.zeros(Cout), None
        for i, g in enumerate(gs):
            gt = torch.tensor(g.astype(F64)[None])
            bt = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
            torch.nn.functional.conv2d(torch.zeros((1, 1, H, W), dtype=torch.float64), torch.zeros((Cout, 1, 3, 3), dtype=torch.float64), bt, padding=1).backward(gt)
            tot64, mag = tot64 + g.astype(F64).sum((1, 2)), mag + np.abs(g.astype(F64)).sum((1, 2))
            assert np.allclose(bt.grad.numpy(), g.astype(F64).sum((1, 2)), rtol=1e-12, atol=1e-12)
            for p in g.reshape(Cout, -1).T:
                seq = seq + p
            db = K.bias_grad_f32(g, db)
            bound = (H * W * (i + 1) + (i + 1) + 1) * K.U23 * mag
            if exact:
                assert (mag < 2.0 ** 24).all() and _same(seq, tot64.astype(F32)) and _same(db, tot64.astype(F32))
            else:
                _note("conv_bias_grad (sequential)", _ratio(np.abs(seq.astype(F64) - tot64), bound))
                _note("conv_bias_grad (its order)", _ratio(np.abs(db.astype(F64) - tot64), bound))


# ---- the pool's routing --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W", K.POOL_SHAPES)
def test_pool_routing(C, H, W):
    x, gy = K.pool_inputs(C, H, W)
    if x.size >= 32:
        assert np.isnan(x).any() and np.isneginf(x).any() and (R.bits(x) == 0x80000000).any()
    for relu_mask in (0, 1):
        dx = K.pool_backward(x, gy, relu_mask)
        with np.errstate(invalid="ignore"):
            assert _same(dx, TT.maxpool_backward_np(x, gy, relu_mask))
        assert ((dx != 0).reshape(C, -1).sum(1) <= gy[0].size).all()   # at most one cell per window
        if relu_mask:
            with np.errstate(invalid="ignore"):
                assert (R.bits(dx)[~(x > 0)] == 0).all()
    # autograd on a tie-free, NaN-free map
    rng = np.random.default_rng([C, H, W])
    xs = rng.permutation(C * H * W).reshape(C, H, W).astype(F64) - C * H * W / 3
    xt = torch.tensor(xs[None], requires_grad=True)
    torch.nn.functional.max_pool2d(xt, 2, 2, ceil_mode=True).backward(torch.tensor(gy.astype(F64)[None]))
    grad = xt.grad.numpy()[0].astype(F32)
    assert _same(K.pool_backward(xs, gy, 0), grad)
    assert _same(K.pool_backward(xs, gy, 1), np.where(xs > 0, grad, F32(0)))   # the mask of the cell the value went to


# ---- the segmented forms -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.SEG_CASES)
def test_segmented_reference_and_bounds(case):
    nseg, N, Kk, B, Mp = case
    g, x = K.seg_inputs(nseg, N, Kk, B)
    g2, x2 = g.reshape(nseg * B, N), x.reshape(nseg * B, Kk)
    n = nseg * B + nseg
    dW64, db64 = g2.astype(F64).T @ x2.astype(F64), g2.astype(F64).sum(0)
    _note("segmented dW", _ratio(np.abs(R.seq_dot_f32(g2, x2).astype(F64) - dW64), R.dot_bound(g2, x2, n)))
    seq = np.zeros(N, F32)
    for row in g2:
        seq = seq + row
    bound = (n + 1) * K.U23 * np.abs(g2.astype(F64)).sum(0)
    _note("segmented db (sequential)", _ratio(np.abs(seq.astype(F64) - db64), bound))
    _note("segmented db (its order)", _ratio(np.abs(K.seg_bias_f32(g).astype(F64) - db64), bound))
    gp = K.seg_pack(g, Mp, K.cdiv(N, 8), lane_fill=R.SENT_F, row_fill=R.SENT_F)
    assert gp.shape == (K.cdiv(N, 8), nseg * Mp, 8)
    s, m, c = nseg - 1, B - 1, N - 1
    assert gp[c // 8, s * Mp + m, c % 8] == g[s, m, c] and (R.bits(gp) == R.SENT).sum() == gp.size - g.size
    if nseg <= 64:   # one block of leaves: with <= 1 segment the tree adds only zeros
        assert nseg > 1 or _same(K.seg_bias_f32(g), R.bias_sum_f32(g[0]))


def test_every_parameter_value_of_the_segmented_cases_appears():
    for i, want in enumerate(((1, 8, 9, 49, 64, 65, 130), (1, 7, 48, 129), (8, 100, 112, 264), (1, 2, 3, 7, 8, 9, 70), (128, 256))):
        assert {c[i] for c in K.SEG_CASES} == set(want)
    for nseg in (9, 65, 130):
        assert any(c[0] == nseg and c[1] % 8 for c in K.SEG_CASES)


def test_scale_inputs_hold_the_special_values():
    for n in K.SCALE_N:
        v = K.scale_inputs(n)
        assert v.shape == (n,)
        if n >= 1023:
            b = R.bits(v)
            assert np.isnan(v).any() and np.isinf(v).any() and (b == 0).any() and (b == 0x80000000).any()
            assert ((np.abs(v) > 0) & (np.abs(v) < 2.0 ** -126)).any()
    assert K.SCALE_N[-1] // 4 > 256 * 4096 and K.SCALE_N[-1] % 4 == 1   # a second grid-stride trip and a tail
