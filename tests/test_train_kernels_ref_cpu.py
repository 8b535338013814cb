"""tests/train_kernels_np.py checked on the CPU: the layout helpers are inverses of each other, the float64 references agree with PyTorch-CPU
autograd in float64, and — for every input set of tests/test_gpu_train_kernels_numerics.py — a plain NumPy fp32 evaluation (sequential sum)
of dW, db and dx stays inside the derived bounds, so the bounds are known to be satisfiable by a correct fp32 implementation before any
kernel is judged against them."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_kernels_np as R  # noqa: E402

F32, F64 = np.float32, np.float64


def _same(a, b):
    return np.array_equal(R.bits(a), R.bits(b))


# ---- layouts -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,Mp", [(1, 1, 128), (5, 8, 7), (33, 35, 256), (130, 129, 384)])
def test_c8_pack_unpack(M, N, Mp):
    a = R.draw(np.random.default_rng([M, N]), (M, N))
    c8 = R.c8_pack(a, Mp, lane_fill=R.SENT_F, row_fill=R.SENT_F)
    assert c8.shape == (R.cdiv(N, 8), Mp, 8)
    assert _same(R.c8_unpack(c8, M, N), a)
    flat = c8.reshape(-1)
    for m, n in ((0, 0), (M - 1, N - 1), (M // 2, N // 2)):  # the header's address rule
        assert flat[((n // 8) * Mp + m) * 8 + n % 8] == a[m, n]
    assert (R.bits(c8) == R.SENT).sum() == c8.size - M * N  # everything that is no element holds the fill


@pytest.mark.parametrize("K,N,inner", [(8, 1, 1), (96, 35, 1), (264, 129, 1), (48, 7, 3), (1568, 35, 49)])
def test_linear_pack_unpack(K, N, inner):
    w = R.draw(np.random.default_rng([K, N, inner]), (N, K), zero_frac=0.0)
    pk = R.lin_pack(w, inner, fill=R.SENT_F)
    assert pk.shape == (R.k64(K) // 8, R.lin_np(N), 8)
    assert _same(R.lin_unpack(pk, K, N, inner), w)
    valid = R.lin_valid(K, N, inner)
    assert valid.sum() == K * N and (R.bits(pk)[~valid] == R.SENT).all() and (R.bits(pk)[valid] != R.SENT).all()
    kidx = R.lin_k_index(K, inner)
    assert sorted(kidx[kidx < K].tolist()) == list(range(K))  # a permutation of the layer's k
    for q in (0, kidx.shape[0] // 3, K // 8 - 1):
        for j in (0, 5):
            assert kidx[q, j] == ((q // inner) * 8 + j) * inner + q % inner
    x = R.draw(np.random.default_rng(7), (3, K), zero_frac=0.0)
    xp = R.x_pack(x, inner, 5)
    # the operand matrix carries the same permutation: the forward GEMM's sum over (chunk, lane) is x W^T
    y = np.einsum("qmj,qnj->mn", xp[:, :3].astype(F64), R.lin_pack(w, inner).astype(F64)[:, :N])
    assert np.allclose(y, x.astype(F64) @ w.astype(F64).T, rtol=1e-12, atol=0)


@pytest.mark.parametrize("Cin,Cout", [(3, 5), (8, 128), (12, 130)])
def test_conv_pack_unpack(Cin, Cout):
    w = R.draw(np.random.default_rng([Cin, Cout]), (Cout, Cin, 3, 3), zero_frac=0.0)
    pk = R.conv_pack(w, fill=R.SENT_F)
    assert pk.shape == (R.cdiv(Cin, 8), 9, R.conv_coutp(Cout), 8)
    assert _same(R.conv_unpack(pk, Cin, Cout), w)
    valid = R.conv_valid(Cin, Cout)
    assert valid.sum() == w.size and (R.bits(pk)[~valid] == R.SENT).all()
    co, ci, ky, kx = Cout - 1, Cin - 1, 2, 1
    assert pk[ci // 8, ky * 3 + kx, co, ci % 8] == w[co, ci, ky, kx]


def test_c8p_pack():
    x = R.draw(np.random.default_rng(1), (12, 9, 3), zero_frac=0.0)
    m = R.c8p_pack(x, fill=R.SENT_F)
    assert m.shape == (2, 18, 34, 8)
    inner = R.c8p_interior(12, 9, 3)
    assert inner.sum() == 2 * 9 * 3 * 8
    assert m[1, 1 + 4, 1 + 2, 3] == x[11, 4, 2]
    assert (R.bits(m)[~inner] == R.SENT).all() and (R.bits(m)[inner] == R.SENT).sum() == 4 * 9 * 3  # the pad channels 12..15


# ---- float64 references against autograd ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,K,k", [(2, 1, 0), (7, 3, 1), (81, 2, 1)])
@pytest.mark.parametrize("norm", [0, 1])
def test_loss_ref_vs_autograd(C, K, k, norm):
    B = 37
    head, rois, gt, labels = R.loss_inputs(C, K, k, B)
    bw = 1.5
    loss, g = R.loss_ref64(head, C, K, k, rois, gt, labels, R.MEAN4, R.STD4, norm, bw)
    y = torch.as_tensor(R.clamp_labels(labels, C))
    h = torch.tensor(head.astype(F64), requires_grad=True)
    r, t = torch.tensor(rois.astype(F64)), torch.tensor(gt.astype(F64))
    L_cls = torch.nn.CrossEntropyLoss()(h[:, k * C:(k + 1) * C], y)
    fg = torch.nonzero(y > 0)[:, 0]
    xc, yc, w, hh = (r[:, 0] + r[:, 2]) * 0.5, (r[:, 1] + r[:, 3]) * 0.5, r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
    xtc, ytc, wt, ht = (t[:, 0] + t[:, 2]) * 0.5, (t[:, 1] + t[:, 3]) * 0.5, t[:, 2] - t[:, 0], t[:, 3] - t[:, 1]
    tg = torch.stack([(xtc - xc) / w, (ytc - yc) / hh, torch.log(wt / w), torch.log(ht / hh)], 1)
    if norm:
        tg = (tg - torch.tensor(np.asarray(R.MEAN4, F32).astype(F64))) / torch.tensor(np.asarray(R.STD4, F32).astype(F64))
    cols = K * C + 4 * y[fg][:, None] + torch.arange(4)[None, :]
    L_box = bw * torch.nn.SmoothL1Loss(reduction="sum")(h[fg[:, None], cols], tg[fg]) / B
    (L_cls + L_box).backward()
    lc, lb = float(L_cls.detach()), float(L_box.detach())
    assert abs(loss[0] - lc) <= 1e-13 * abs(lc) and abs(loss[1] - lb) <= 1e-13 * abs(lb)
    assert np.abs(g - h.grad.numpy()).max() <= 1e-15
    # the fp32 restatement is the same function: close to float64, and exactly zero where the contract says +0.0
    l32, g32 = R.loss_f32(head, C, K, k, rois, gt, labels, R.MEAN4, R.STD4, norm, bw)
    assert np.abs(l32 - loss).max() <= 1e-5 * np.abs(loss).max() and np.abs(g32 - g).max() <= 1e-6
    assert (R.bits(g32)[g == 0] == 0).all()


def test_linear_refs_vs_autograd():
    N, K, B = 35, 96, 33
    g, w, act = R.dgrad_inputs(N, K, B)
    x = torch.tensor(R.draw(np.random.default_rng(5), (B, K)).astype(F64), requires_grad=True)
    W = torch.tensor(w.astype(F64), requires_grad=True)
    b = torch.zeros(N, dtype=torch.float64, requires_grad=True)
    ((x @ W.t() + b) * torch.tensor(g.astype(F64))).sum().backward()
    g64, w64 = g.astype(F64), w.astype(F64)
    assert np.abs(W.grad.numpy() - g64.T @ x.detach().numpy()).max() <= 1e-12
    assert np.abs(b.grad.numpy() - g64.sum(0)).max() <= 1e-12
    assert np.abs(x.grad.numpy() - g64 @ w64).max() <= 1e-12


# ---- the bounds are satisfiable: a sequential fp32 evaluation of every GPU input set ------------------------------------------------------
def test_wgrad_bound_holds_for_sequential_fp32():
    worst = 0.0
    for N, K, inner, B in R.wgrad_cases():
        g, x = R.wgrad_inputs(N, K, inner, B)
        dw = R.seq_dot_f32(g, x)  # [N, K]
        ref, bound = g.astype(F64).T @ x.astype(F64), R.dot_bound(g, x, B)
        err = np.abs(dw.astype(F64) - ref)
        assert (err <= bound).all(), (N, K, inner, B)
        nz = bound > 0
        worst = max(worst, float((err[nz] / bound[nz]).max()) if nz.any() else 0.0)
        assert (dw[~nz] == 0).all()
    print("\nACC sequential fp32 dW: largest error / bound = %.3f" % worst)
    assert worst > 0  # the comparison is not vacuous


def test_bias_bound_holds_for_sequential_and_documented_order():
    worst = 0.0
    for N in R.BIAS_N:
        for B in R.BIAS_B:
            g = R.bias_inputs(N, B)
            ref, bound = g.astype(F64).sum(0), (B + 1) * R.U23 * np.abs(g.astype(F64)).sum(0)
            seq = np.zeros(N, F32)
            for m in range(B):
                seq = seq + g[m]
            for got in (seq, R.bias_sum_f32(g)):
                err = np.abs(got.astype(F64) - ref)
                assert (err <= bound).all(), (N, B)
                nz = bound > 0
                worst = max(worst, float((err[nz] / bound[nz]).max()) if nz.any() else 0.0)
    print("\nACC fp32 db (sequential and 32-slot tree): largest error / bound = %.3f" % worst)


def test_dgrad_bound_holds_for_sequential_fp32():
    worst = 0.0
    for N, K, B in R.dgrad_cases():
        g, w, act = R.dgrad_inputs(N, K, B)
        dx = R.seq_dot_f32(g.T, w)  # [B, K]
        ref, bound = g.astype(F64) @ w.astype(F64), R.dot_bound(g.T, w, N, extra=4)
        err = np.abs(dx.astype(F64) - ref)
        assert (err <= bound).all(), (N, K, B)
        nz = bound > 0
        worst = max(worst, float((err[nz] / bound[nz]).max()) if nz.any() else 0.0)
        for kind in (act > 0, act == 0, act < 0, np.isnan(act)):  # every kind of activation the GPU test speaks of is present from B * K >= 64 on
            assert kind.any() or B * K < 64
    print("\nACC sequential fp32 dx: largest error / bound = %.3f" % worst)


def test_documented_orders_on_small_examples():
    g = np.arange(1, 67, dtype=F32).reshape(66, 1)  # 66 rows: slots 0 and 1 get three rows
    assert R.bias_sum_f32(g)[0] == g.sum()  # small integers: exact in any order
    assert R.block_reduce_f32(np.arange(300, dtype=F32)) == F32(300 * 299 / 2)
    w, v = R.sgd_f32([1.0], [0.5], [0.25], 0.5, 0.5, 0.25)
    assert v[0] == F32(0.5 * 0.5 + (0.25 + 0.25 * 1.0)) and w[0] == F32(1.0 - 0.5 * v[0])
    w, v = R.sgd_f32([0.0], [0.0], [3.0], 1.0, 0.0, 0.0)  # the gradient tier: v ends as dW, w as -dW
    assert v[0] == 3 and w[0] == -3
    y, keep = R.dropout_f32(np.ones((4, 9), F32), 0.0, R.SEED, 0, 0)
    assert keep.all() and (y == 1).all()
    y, keep = R.dropout_f32(np.full((64, 96), 3.0, F32), 0.5, R.SEED, 2 ** 31 + 5, 1)
    assert 0.4 < keep.mean() < 0.6 and (y[keep] == 6).all() and (R.bits(y)[~keep] == 0).all()
