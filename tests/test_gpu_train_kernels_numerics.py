"""The head-training kernels (multipathnet_amd/csrc/train.hip), one launch at a time, against float64 and against NumPy restatements of what
train.h documents operation by operation: train_loss, sgd_wgrad_c8, sgd_bias_c8, linear_dgrad_c8, dropout_c8, the layout helpers, conv_sgd,
vec_sgd and relu_mask_c8p.  Until now they were reachable only through mpn_frcnn_train_step on one tiny network (K6 = 1568, fc_dim <= 128,
C <= 7, B <= 200, read back through unpack_linear_weights, which skips every pad lane).

The kernels are called through the mpn_debug_* pass-throughs of train_debug.hip (debug flavour only): raw device pointers in the kernels'
own layouts, the product's host wrappers, and an element count per buffer that turns a layout mistake of this file into MPN_EINVAL.  The
layouts and references are tests/train_kernels_np.py's (checked on the CPU in tests/test_train_kernels_ref_cpu.py).

Common setup.  Every device buffer sits between two guard zones of 256 floats holding a sentinel NaN (0x7FA5A5A5) that must survive every
launch.  Regions of an output the contract says are not written hold the sentinel and must keep its bits; regions of an input the contract
says are not read (rows >= B; lanes n >= N of g's last chunk for sgd_wgrad_c8 and linear_dgrad_c8; rows n >= N of the pack for
linear_dgrad_c8) hold NaN.  Real values have magnitudes in [2^-6, 2^3] plus exact zeros.  Every case runs twice: the same bits.

Tiers.
  bit-exact   the build uses -ffp-contract=off, so optim.sgd's chain (gr = f32(dW + f32(wd w)), v' = f32(f32(mom v) + gr),
              w' = f32(w - f32(lr v'))), sgd_bias_kernel's summation order (32 slot sums, then the tree 16..1), dropout's f32(x * scale), the
              ReLU / dropout mask and scale of linear_dgrad_c8, every +0.0 of train_loss's gradient, its clamp boundaries and its box loss on
              boundary rows, and all layout kernels are reproduced bit for bit.
  derived     a length-n fp32 dot product: |r - r64| <= (n + 1) * 2^-23 * sum |a_i| |b_i| (tests/train_kernels_np.py says why); n = B for
              dW and db, n + 4 with n = N for dx (three more additions join the four waves' partial sums).
  yardstick   train_loss's softmax gradient, box gradient through logf, and the two losses: no derived bound; judged against float64 beside
              a NumPy fp32 restatement of the same chain on max and rms with MARGIN = 2.0, the factor tests/test_gpu_train.py grants this
              kernel through the whole step; where the restatement's error is zero the device's must be zero.

What the module found.  unpack_linear_weights took any (K, inner): with inner > 1 and K no multiple of 8 * inner a k < K maps to a chunk past
K64 / 8 and the kernel reads outside the pack (K = 1000, inner = 49: chunk 146 of 128).  No caller in the library passes such a pair, but the
wrapper now refuses it as pack_linear_weights always did (test_refusals).  The kernels themselves met every check below.

MEASURED on the MI355X (largest observed error / bound per family, from the ACC lines; DESIGN.md section 13.8 has the same table):
  sgd_wgrad_c8 dW      0.294 (N 35, K 264, B 2); N = 1 / 35 / 128 / 129: 0.215 / 0.294 / 0.284 / 0.285   (a sequential fp32 chain on the CPU: 0.300)
  sgd_bias_c8 db       0.019 (N 130, B 31); the device's bits are the emulated order's in all 30 cases    (CPU, sequential and tree: 0.038)
  linear_dgrad_c8 dx   0.166 (N 3); N = 1 / 2 / 3 / 7 / 35 / 130: 0.099 / 0.156 / 0.166 / 0.148 / 0.045 / 0.010   (CPU sequential: 0.200)
  train_loss, device error / NumPy-fp32 error against float64 (max ratio, rms ratio), MARGIN 2.0:
    softmax gradient per (C, K, k, norm) over all B    1.00, 0.98 - 1.08
    box gradient per (C, K, k, norm) over all B        0.63 - 1.00, 0.92 - 1.00
    L_cls / L_box over all 96 cases                    0.97, 0.92 / 1.00, 1.00
    saturated (logits +-80) L_cls, softmax gradient    1.00, 1.00 each
  No ratio exceeds 1.08: expf and logf were not measured on their own.  The module's wall time is under 2 s.

Mutations tried on scratch copies of the debug library (MI355X; each in bounds by construction), with the tests that fail on each:
  sgd_wgrad_kernel's load guard as m < a.B - 1 (the last row dropped)        test_sgd_wgrad (32 of 33 cases)
  sgd_wgrad_kernel's gr without the wd * w term                              test_sgd_wgrad (33 of 33)
  dropout_c8_kernel without its `< N` check                                  test_dropout (all four rates)
  linear_dgrad_kernel's ne = nb + n_per_wave (the last wave runs past N)     test_linear_dgrad (all N; the NaN rows of the pack reach dx)
  linear_dgrad_kernel's mask as act >= 0                                     test_linear_dgrad (all N)
  train_loss_kernel's row loop stopped after one trip                        test_train_loss (all 8) and the three other loss tests
  sgd_bias_kernel's slot sums taken descending                               test_sgd_bias
  conv_sgd_kernel without its ci >= Cin guard                                test_conv_sgd_and_unpack_conv_weights[3-5], [12-130]
The last-wave mutant first slipped through at N = 7, 35 and 130: its NaN went through max() and `<=`, which are both blind to one.  _acc
now refuses a non-finite error itself.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dropout_np as D  # noqa: E402
import train_kernels_np as R  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENT, SENT_F = R.SENT, R.SENT_F
GUARD = 256
MPN_EINVAL = -1
MARGIN = 2.0  # tests/test_gpu_train.py's, for train_loss's exp / log parts only
BW = 1.5      # bbox_weight
cf, ci, cs, u32, vp = C.c_float, C.c_int, C.c_size_t, C.c_uint32, C.c_void_p
SGD_PARAMS = ((1e-3, 0.9, 5e-4), (0.25, 0.5, 0.0), (0.0, 0.9, 5e-4))


@functools.lru_cache(maxsize=None)
def _dbg():
    from multipathnet_amd import _lib
    lib = _lib.load("debug")
    b = [vp, cs]  # a buffer and its element count
    f4 = C.POINTER(C.c_float * 4)
    lib.mpn_debug_train_loss.argtypes = b + [ci, ci, ci, ci] + b + b + b + [f4, f4, ci, cf] + b + [ci] + b
    lib.mpn_debug_sgd_wgrad_c8.argtypes = b + [ci] + b + [ci, ci, ci, ci, ci] + b + b + [cf, cf, cf]
    lib.mpn_debug_sgd_bias_c8.argtypes = b + [ci, ci, ci] + b + b + [cf, cf]
    lib.mpn_debug_linear_dgrad_c8.argtypes = b + [ci, ci, ci] + b + [ci] + b + b + [ci, cf]
    lib.mpn_debug_dropout_c8.argtypes = b + [ci, ci, ci, u32, u32, u32, u32, u32, cf]
    lib.mpn_debug_c8_rows_to_rowmajor.argtypes = b + [ci, ci, ci] + b
    lib.mpn_debug_pack_linear_weights.argtypes = b + b + [ci, ci, ci] + b + b
    lib.mpn_debug_unpack_linear_weights.argtypes = b + b + [ci, ci, ci, ci, ci] + b + b
    lib.mpn_debug_conv_sgd.argtypes = b + b + b + [ci, ci, cf, cf, cf]
    lib.mpn_debug_vec_sgd.argtypes = b + b + b + [ci, cf, cf]
    lib.mpn_debug_relu_mask_c8p.argtypes = b + b + [ci, ci, ci]
    lib.mpn_debug_unpack_conv_weights.argtypes = b + b + [ci, ci] + b + b
    return lib


def _err():
    return _dbg().mpn_last_error().decode()


def _ok(rc):
    assert rc == 0, (rc, _err())


def _sent(*shape):
    return np.full(shape, SENT, np.uint32).view(F32)


def _same(a, b):
    return np.array_equal(R.bits(a), R.bits(b))


def _same_nanpos(got, ref):
    """bit equality where the reference is a number; a NaN wherever it has one (the host's and the device's NaN results differ in bits)"""
    got, ref = np.asarray(got, F32), np.asarray(ref, F32)
    n = np.isnan(ref)
    return np.array_equal(np.isnan(got), n) and np.array_equal(R.bits(got)[~n], R.bits(ref)[~n])


def _is_sent(a):
    return bool((R.bits(a) == SENT).all())


class Buf(object):
    """a device buffer between two guard zones of GUARD sentinel floats; .a = (pointer, element count) as the entries take them"""

    def __init__(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.dtype in (np.float32, np.int32)
        self.shape, self.dtype, self.n = arr.shape, arr.dtype, arr.size
        host = np.full(self.n + 2 * GUARD, SENT, np.uint32)
        host[GUARD:GUARD + self.n] = arr.reshape(-1).view(np.uint32)
        self.t = torch.from_numpy(host.view(np.int32)).to(torch.device("cuda", 0))
        self.ptr = self.t.data_ptr() + 4 * GUARD
        assert self.ptr % 16 == 0
        self.a = (vp(self.ptr), self.n)

    def short(self, by=1):
        return (vp(self.ptr), self.n - by)

    def read(self):
        torch.cuda.synchronize()
        h = self.t.cpu().numpy().view(np.uint32)
        assert (h[:GUARD] == SENT).all() and (h[GUARD + self.n:] == SENT).all(), "a launch wrote into a guard zone"
        return h[GUARD:GUARD + self.n].view(self.dtype).reshape(self.shape).copy()


NULL = (None, 0)


def twice(call):
    """every case runs twice on fresh buffers: the same bits.  call() -> tuple of numpy arrays"""
    a, b = call(), call()
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), "two runs differ"
    return a


def _acc(tag, err, bound):
    """largest err / bound over the elements with a non-zero bound; where the bound is 0 (all products zero) the error must be 0"""
    nz = bound > 0
    assert np.isfinite(err).all(), tag + ": a NaN or inf in the result"  # (max() and `<=` are both blind to a NaN)
    assert (err[~nz] == 0).all(), tag
    ratio = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    print("ACC %-44s err / bound = %.3f" % (tag, ratio))
    assert ratio <= 1.0, tag
    return ratio


# ---- sgd_wgrad_c8 ------------------------------------------------------------------------------------------------------------------------
G_MP, X_MP = 256, 384


def _run_wgrad(g_c8, x_c8, w0, v0, B, N, K, inner, lr, mom, wd):
    def call():
        gb, xb, wb, vb = Buf(g_c8), Buf(x_c8), Buf(w0), Buf(v0)
        _ok(_dbg().mpn_debug_sgd_wgrad_c8(*gb.a, G_MP, *xb.a, X_MP, B, N, K, inner, *wb.a, *vb.a, lr, mom, wd))
        w, v = wb.read(), vb.read()
        assert _same(gb.read(), g_c8) and _same(xb.read(), x_c8)
        return w, v
    return twice(call)


@pytest.mark.parametrize("N,K,inner,B", R.wgrad_cases())
def test_sgd_wgrad(dev, N, K, inner, B):
    g, x = R.wgrad_inputs(N, K, inner, B)
    g_c8 = R.c8_pack(g, G_MP, lane_fill=SENT_F, row_fill=SENT_F)          # lanes n >= N and rows >= B: never read
    x_c8 = R.x_pack(x, inner, X_MP, lane_fill=SENT_F, row_fill=SENT_F)    # pad k lanes: read and discarded
    valid = R.lin_valid(K, N, inner)
    assert x_c8.shape[0] == R.k64(K) // 8 and valid.shape == (R.k64(K) // 8, R.lin_np(N), 8)
    ref, bound = g.astype(F64).T @ x.astype(F64), R.dot_bound(g, x, B)
    rng = np.random.default_rng([N, K, inner, B, 9])
    dW = None
    for fill in (F32(0.0), SENT_F):  # the packing's +0.0, then the sentinel: "not touched", not "rewritten"
        z = np.full(valid.shape, fill, F32)
        z[valid] = 0
        # (a) the gradient: w = v = +0, lr = 1, mom = 0, wd = 0 -> v ends as dW itself
        w1, v1 = _run_wgrad(g_c8, x_c8, z, z, B, N, K, inner, 1.0, 0.0, 0.0)
        assert _same(w1[~valid], z[~valid]) and _same(v1[~valid], z[~valid]), "a pad lane of the pack was written"
        got = R.lin_unpack(v1, K, N, inner)
        err = np.abs(got.astype(F64) - ref)
        ratio = _acc("sgd_wgrad N=%d K=%d inner=%d B=%d" % (N, K, inner, B), err, bound)
        assert ratio <= 1.0
        assert _same(w1[valid], F32(0) - F32(1) * v1[valid])
        assert dW is None or _same(dW[valid], v1[valid])
        dW = v1
        # (b) the optimiser on the same g and x: bit-equal to the emulated chain fed with (a)'s dW bits
        w0, v0 = z.copy(), z.copy()
        w0[valid], v0[valid] = R.draw(rng, int(valid.sum())), R.draw(rng, int(valid.sum()))
        for lr, mom, wd in SGD_PARAMS:
            w2, v2 = _run_wgrad(g_c8, x_c8, w0, v0, B, N, K, inner, lr, mom, wd)
            ew, ev = R.sgd_f32(w0, v0, dW, lr, mom, wd)
            assert _same(w2[valid], ew[valid]) and _same(v2[valid], ev[valid]), (lr, mom, wd)
            assert _same(w2[~valid], z[~valid]) and _same(v2[~valid], z[~valid])
            if lr == 0.0:
                assert _same(w2[valid], w0[valid])


# ---- sgd_bias_c8 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", R.BIAS_N)
def test_sgd_bias(dev, N):
    NP, Mp = R.lin_np(N), 160
    worst = 0.0
    for B in R.BIAS_B:
        g = R.bias_inputs(N, B)
        g_c8 = R.c8_pack(g, Mp, lane_fill=0.0, row_fill=SENT_F)  # pad lanes as train_loss writes them; rows >= B: never read
        rng = np.random.default_rng([N, B, 8])
        b0, vb0 = _sent(NP), _sent(NP)
        b0[:N], vb0[:N] = R.draw(rng, N), R.draw(rng, N)
        db = R.bias_sum_f32(g)
        ref, bound = g.astype(F64).sum(0), (B + 1) * R.U23 * np.abs(g.astype(F64)).sum(0)
        worst = max(worst, _acc("sgd_bias emulated order N=%d B=%d" % (N, B), np.abs(db.astype(F64) - ref), bound))
        for lr, mom in ((1.0, 0.0), (1e-3, 0.9), (0.0, 0.9)):
            def call():
                gb, bb, vb = Buf(g_c8), Buf(b0), Buf(vb0)
                _ok(_dbg().mpn_debug_sgd_bias_c8(*gb.a, Mp, B, N, *bb.a, *vb.a, lr, mom))
                gb.read()
                return bb.read(), vb.read()
            b1, v1 = twice(call)
            eb, ev = R.sgd_bias_f32(b0[:N], vb0[:N], db, lr, mom)
            assert _same(v1[:N], ev) and _same(b1[:N], eb), (N, B, lr, mom)
            assert _is_sent(b1[N:]) and _is_sent(v1[N:])
            if lr == 0.0:  # b keeps its bits, vb is still updated
                assert _same(b1[:N], b0[:N]) and (N < 7 or not _same(v1[:N], vb0[:N]))
            if mom == 0.0:  # v' = f32(f32(0 * v) + db): the device's sum itself against float64
                worst = max(worst, _acc("sgd_bias device N=%d B=%d" % (N, B), np.abs(v1[:N].astype(F64) - ref), bound))
        assert worst <= 1.0


# ---- linear_dgrad_c8 ---------------------------------------------------------------------------------------------------------------------
DG_GMP, DG_XMP = 136, 104
SCALE_03 = F32(1.0) / (F32(1.0) - F32(0.3))


@pytest.mark.parametrize("N", R.DGRAD_N)
def test_linear_dgrad(dev, N):
    worst = 0.0
    for K in R.DGRAD_K:
        for B in R.DGRAD_B:
            g, w, act = R.dgrad_inputs(N, K, B)
            g_c8 = R.c8_pack(g, DG_GMP, lane_fill=SENT_F, row_fill=SENT_F)
            wpk = R.lin_pack(w, 1, fill=SENT_F)  # rows n >= N of the pack: never read
            act_c8 = R.c8_pack(act, DG_XMP, row_fill=SENT_F)
            nch = K // 8
            out = {}
            for scale in (F32(1.0), F32(2.0), SCALE_03):
                def call():
                    gb, wb, ab, db = Buf(g_c8), Buf(wpk), Buf(act_c8), Buf(_sent(nch + 1, DG_XMP, 8))
                    _ok(_dbg().mpn_debug_linear_dgrad_c8(*gb.a, DG_GMP, B, N, *wb.a, K, *ab.a, *db.a, DG_XMP, float(scale)))
                    gb.read(), wb.read(), ab.read()
                    return (db.read(),)
                dx = twice(call)[0]
                assert _is_sent(dx[:, B:]) and _is_sent(dx[nch:]), "rows >= B or chunks >= ceil(K / 8) were written"
                out[float(scale)] = R.c8_unpack(dx, B, K)
            r1 = out[1.0]
            assert np.isfinite(r1).all(), "a NaN reached dx: a row >= N of the pack, a lane >= N of g or a NaN activation was used"
            on = act > 0  # NaN > 0 is false: +0.0 there too
            assert (R.bits(r1)[~on] == 0).all(), "not exactly +0.0 where act <= 0, -0.0 or NaN"
            ref, bound = g.astype(F64) @ w.astype(F64), R.dot_bound(g.T, w, N, extra=4)
            if on.any():
                err = np.abs(r1.astype(F64) - ref)
                worst = max(worst, _acc("linear_dgrad N=%d K=%d B=%d" % (N, K, B), err[on], bound[on]))
            assert (act[on] >= F32(2.0 ** -126)).all() and (act == F32(2.0 ** -126)).any() or B * K < 64
            assert _same(out[2.0], r1 * F32(2.0)), "scale 2 is not twice the scale-1 bits"
            assert _same(out[float(SCALE_03)], r1 * SCALE_03), "scale 1 / (1 - 0.3f) is not f32(bits * scale)"
    assert worst <= 1.0


# ---- train_loss --------------------------------------------------------------------------------------------------------------------------
def _run_loss(head, rois, gt, labels, B, C_, K, k, norm):
    ld = (K + 4) * C_
    chunks, Mp = R.cdiv(ld, 8), R.round_up(B, 128) + 128
    m4, s4 = (C.c_float * 4)(*R.MEAN4), (C.c_float * 4)(*R.STD4)

    def call():
        hb, rb, tb, lb = Buf(head), Buf(rois), Buf(gt), Buf(np.asarray(labels, np.int32))
        gb, ob = Buf(_sent(chunks, Mp, 8)), Buf(_sent(4))
        _ok(_dbg().mpn_debug_train_loss(*hb.a, B, C_, K, k, *rb.a, *tb.a, *lb.a, m4, s4, norm, BW, *gb.a, Mp, *ob.a))
        hb.read(), rb.read(), tb.read(), lb.read()
        return ob.read(), gb.read()
    loss, g_c8 = twice(call)
    assert _is_sent(loss[2:]) and _is_sent(g_c8[:, B:]), "rows >= B of the gradient (or floats past the two losses) were written"
    full = g_c8[:, :B].transpose(1, 0, 2).reshape(B, chunks * 8)
    assert (R.bits(full[:, ld:]) == 0).all(), "pad lanes of the last chunk are not +0.0"
    return loss[:2], full[:, :ld].copy()


@functools.lru_cache(maxsize=None)
def _loss_case(C_, K, k, B, norm, kind="mixed"):
    """device result and the two references of one input set, computed once -> (inputs, loss, g, loss64, g64, loss32, g32)"""
    if kind == "boundary":
        inp = R.loss_boundary_inputs(C_, K, k, B)
    else:
        inp = R.loss_inputs(C_, K, k, B, all_bg=kind == "all_bg", saturated=kind == "saturated")
    head, rois, gt, labels = inp
    loss, g = _run_loss(head, rois, gt, labels, B, C_, K, k, norm)
    l64, g64 = R.loss_ref64(head, C_, K, k, rois, gt, labels, R.MEAN4, R.STD4, norm, BW)
    l32, g32 = R.loss_f32(head, C_, K, k, rois, gt, labels, R.MEAN4, R.STD4, norm, BW)
    return inp, loss, g, l64, g64, l32, g32


def _judge(tag, r, r64, r32):
    """tests/test_gpu_train.py's rule: max and rms of |r - r64| within MARGIN of the fp32 restatement's"""
    r, r64, r32 = np.asarray(r, F64).reshape(-1), np.asarray(r64, F64).reshape(-1), np.asarray(r32, F64).reshape(-1)
    e, y = np.abs(r - r64), np.abs(r32 - r64)
    em, er, ym, yr = float(e.max()), float(np.sqrt((e * e).mean())), float(y.max()), float(np.sqrt((y * y).mean()))
    print("ACC %-44s max e %.3g / numpy-fp32 %.3g = %.2f   rms e %.3g / %.3g = %.2f" %
          (tag, em, ym, em / ym if ym else (0.0 if em == 0 else np.inf), er, yr, er / yr if yr else (0.0 if er == 0 else np.inf)))
    return em <= MARGIN * ym and er <= MARGIN * yr


def _zero_mask(labels, B, C_, K, k):
    """the columns train.h says are exactly +0.0: the other classifiers', the box columns of every class but the label's, all box columns
    of background rows"""
    y = R.clamp_labels(labels, C_)
    m = np.ones((B, (K + 4) * C_), bool)
    m[:, k * C_:(k + 1) * C_] = False
    for i in np.nonzero(y > 0)[0]:
        m[i, K * C_ + 4 * y[i]:K * C_ + 4 * y[i] + 4] = False
    return m


@pytest.mark.parametrize("C_,K,k", R.LOSS_CKK)
def test_train_loss(dev, C_, K, k):
    for norm in (1, 0):
        e_cls, e_box = [[], [], []], [[], [], []]
        for B in R.LOSS_B:
            (head, rois, gt, labels), loss, g, l64, g64, l32, g32 = _loss_case(C_, K, k, B, norm)
            zero = _zero_mask(labels, B, C_, K, k)
            assert (R.bits(g)[zero] == 0).all(), "a column the contract says is +0.0 is not"
            assert np.isfinite(g).all() and np.isfinite(loss).all()
            y = R.clamp_labels(labels, C_)
            if B >= 3:  # -3, C and C + 5 behave as their clamped values: foreground rows of class C - 1 carry box gradients
                assert (np.asarray(labels) < 0).any() and (np.asarray(labels) >= C_).any()
            cls = np.zeros_like(zero)
            cls[:, k * C_:(k + 1) * C_] = True
            box = ~zero & ~cls
            assert box.sum() == 4 * int((y > 0).sum())
            for acc, sel in ((e_cls, cls), (e_box, box)):
                for j, a in enumerate((g, g64, g32)):
                    acc[j].append(np.asarray(a, F64)[sel])
        cat = lambda parts: np.concatenate(parts)
        assert _judge("train_loss cls grad C=%d K=%d k=%d norm=%d" % (C_, K, k, norm), cat(e_cls[0]), cat(e_cls[1]), cat(e_cls[2]))
        assert _judge("train_loss box grad C=%d K=%d k=%d norm=%d" % (C_, K, k, norm), cat(e_box[0]), cat(e_box[1]), cat(e_box[2]))


def test_train_loss_losses_vs_float64(dev):
    """the two losses of every case of test_train_loss, as two vectors (a single sum's error against a single sample of fp32's is no measure)"""
    got, r64, r32 = [], [], []
    for C_, K, k in R.LOSS_CKK:
        for norm in (1, 0):
            for B in R.LOSS_B:
                _, loss, _, l64, _, l32, _ = _loss_case(C_, K, k, B, norm)
                got.append(loss), r64.append(l64), r32.append(l32)
    got, r64, r32 = np.array(got, F64), np.array(r64), np.array(r32, F64)
    assert _judge("train_loss L_cls (all cases)", got[:, 0], r64[:, 0], r32[:, 0])
    assert _judge("train_loss L_box (all cases)", got[:, 1], r64[:, 1], r32[:, 1])


def test_train_loss_boundary_rows(dev):
    """norm = 0 and gt == roi: the targets are exactly 0 and the box outputs walk +-1, +-(1 - 2^-24), +-(1 + 2^-23), +0, -0.  Nothing on that path
    goes through exp or log (logf(1) = 0), so the box gradient f32(gbox * clamp(d)) and loss[1] = the sum of 0.5 d^2 / |d| - 0.5 in the
    documented order are the fp32 restatement's bits."""
    for C_, K, k in ((7, 1, 0), (21, 1, 0), (7, 3, 1), (81, 2, 1)):
        for B in R.LOSS_B:
            (head, rois, gt, labels), loss, g, l64, g64, l32, g32 = _loss_case(C_, K, k, B, 0, "boundary")
            y = R.clamp_labels(labels, C_)
            zero = _zero_mask(labels, B, C_, K, k)
            box = ~zero
            box[:, k * C_:(k + 1) * C_] = False
            assert _same(g[box], g32[box]), (C_, K, k, B)
            assert _same(loss[1], l32[1]), (C_, K, k, B, loss[1], l32[1])
            assert (R.bits(g)[zero] == 0).all()
            if (y > 0).sum() >= 3:  # all eight boundary values were used, the two signed zeros among them
                d = np.concatenate([head[i, K * C_ + 4 * y[i]:K * C_ + 4 * y[i] + 4] for i in np.nonzero(y > 0)[0]])
                assert set(R.bits(d).tolist()) == set(R.bits(R.BOUNDARY_D).tolist())
                gb = g[box]
                gbox = F32(BW) / F32(B)
                assert set(R.bits(gb).tolist()) == {int(R.bits(F32(s) * gbox)[0]) for s in (1, -1, 1 - 2.0 ** -24, -(1 - 2.0 ** -24), 0.0, -0.0)}


def test_train_loss_all_background_and_saturated(dev):
    for C_, K, k in ((7, 1, 0), (81, 2, 1)):
        for B in (2, 257):
            (head, rois, gt, labels), loss, g, l64, g64, l32, g32 = _loss_case(C_, K, k, B, 1, "all_bg")
            assert R.bits(loss[1])[0] == 0, "an all-background batch has loss[1] == +0.0"
            assert (R.bits(g[:, K * C_:]) == 0).all()
    got, r64, r32, gg, gg64, gg32 = [], [], [], [], [], []
    for C_, K, k in ((7, 1, 0), (21, 1, 0), (7, 3, 2), (81, 2, 1)):
        for B in (2, 257, 300):
            (head, rois, gt, labels), loss, g, l64, g64, l32, g32 = _loss_case(C_, K, k, B, 1, "saturated")
            assert np.isfinite(loss).all() and np.isfinite(g).all()
            assert (R.bits(g)[_zero_mask(labels, B, C_, K, k)] == 0).all()
            got.append(loss), r64.append(l64), r32.append(l32)
            sl = slice(k * C_, (k + 1) * C_)
            gg.append(g[:, sl].reshape(-1)), gg64.append(g64[:, sl].reshape(-1)), gg32.append(g32[:, sl].reshape(-1))
    got, r64, r32 = np.array(got, F64), np.array(r64), np.array(r32, F64)
    assert _judge("train_loss saturated L_cls", got[:, 0], r64[:, 0], r32[:, 0])
    assert _judge("train_loss saturated cls grad", np.concatenate(gg), np.concatenate(gg64), np.concatenate(gg32))


# ---- dropout_c8 --------------------------------------------------------------------------------------------------------------------------
DROP_N = (1, 4, 5, 8, 9, 35, 96)
DROP_B = (1, 63, 64, 65)
DROP_MP = 256


def _dropout_x(N, B):
    rng = np.random.default_rng([N, B, 6])
    x = R.draw(rng, (B, N))
    pick = rng.integers(0, 12, (B, N))
    for v, val in enumerate((-0.0, np.inf, -np.inf, np.nan)):
        x[pick == v] = val
    return x


@pytest.mark.parametrize("rate", [0.0, 0.3, 0.5, 0.999])
def test_dropout(dev, rate):
    thr, scale = D.threshold(rate), D.scale(rate)
    kept_n = total_n = 0
    for N in DROP_N:
        nq = R.cdiv(N, 8)
        for B in DROP_B:
            x = _dropout_x(N, B)
            buf = _sent(nq + 1, DROP_MP, 8)
            buf[:nq] = R.c8_pack(x, DROP_MP, lane_fill=SENT_F, row_fill=SENT_F)
            for layer in (0, 1):
                for step in (0, 2 ** 31 + 5):
                    def call():
                        yb = Buf(buf)
                        _ok(_dbg().mpn_debug_dropout_c8(*yb.a, DROP_MP, B, N, thr, R.SEED & 0xFFFFFFFF, R.SEED >> 32, layer, step, float(scale)))
                        return (yb.read(),)
                    y = twice(call)[0]
                    assert _is_sent(y[:, B:]) and _is_sent(y[nq:]), "rows >= B or chunks >= ceil(N / 8) were written"
                    lanes = y[:nq, :B].transpose(1, 0, 2).reshape(B, nq * 8)
                    assert (R.bits(lanes[:, N:]) == 0).all(), "lanes >= N of the last record are not +0.0"
                    exp, keep = R.dropout_f32(x, rate, R.SEED, step, layer)
                    got = lanes[:, :N]
                    assert _same_nanpos(got, exp), (N, B, rate, layer, step)
                    assert (R.bits(got)[~keep] == 0).all()  # dropped: +0.0, also where x is NaN or inf
                    if rate == 0.0:
                        assert keep.all() and _same_nanpos(got, x)
                    kept_n, total_n = kept_n + int(keep.sum()), total_n + keep.size
    assert abs(kept_n / total_n - (1 - rate)) < 0.02  # the inputs did exercise both arms


# ---- layout and element-wise kernels -----------------------------------------------------------------------------------------------------
LIN_CASES = ((8, 1, 1), (96, 35, 1), (264, 129, 1), (48, 7, 3), (1568, 35, 49))


@pytest.mark.parametrize("K,N,inner", LIN_CASES)
def test_pack_unpack_linear_weights(dev, K, N, inner):
    rng = np.random.default_rng([K, N, inner, 5])
    w, b = R.draw(rng, (N, K), zero_frac=0.0), R.draw(rng, N, zero_frac=0.0)
    nq, NP = R.k64(K) // 8, R.lin_np(N)

    def call():
        wb, bb, pk, bp = Buf(w), Buf(b), Buf(_sent(nq, NP, 8)), Buf(_sent(NP))
        _ok(_dbg().mpn_debug_pack_linear_weights(*wb.a, *bb.a, K, N, inner, *pk.a, *bp.a))
        wb.read(), bb.read()
        return pk.read(), bp.read()
    pk, bp = twice(call)
    assert _same(pk, R.lin_pack(w, inner, 0.0)) and _same(bp, R.bias_pack(b)), "pack_linear_weights differs from the layout, pad lanes included"
    # the inverse, from a pack whose pad lanes hold NaN: they are skipped
    src, bsrc = R.lin_pack(w, inner, fill=SENT_F), R.bias_pack(b, fill=SENT_F)
    for n0, n1 in sorted({(0, N), (min(3, N - 1), N), (0, 1), (N - 1, N)}):
        for want_w, want_b in ((1, 1), (1, 0), (0, 1)):
            def call():
                pb, bb = Buf(src), Buf(bsrc)
                wo, bo = Buf(_sent(n1 - n0, K)), Buf(_sent(n1 - n0))
                _ok(_dbg().mpn_debug_unpack_linear_weights(*pb.a, *bb.a, K, N, inner, n0, n1, *(wo.a if want_w else NULL), *(bo.a if want_b else NULL)))
                pb.read(), bb.read()
                return wo.read(), bo.read()
            wo, bo = twice(call)
            assert _same(wo, w[n0:n1]) if want_w else _is_sent(wo), (n0, n1)
            assert _same(bo, b[n0:n1]) if want_b else _is_sent(bo), (n0, n1)


@pytest.mark.parametrize("M,N,Mp", [(1, 1, 128), (5, 8, 7), (33, 35, 256), (130, 129, 384), (300, 405, 301)])
def test_c8_rows_to_rowmajor(dev, M, N, Mp):
    a = R.draw(np.random.default_rng([M, N, Mp]), (M, N), zero_frac=0.0)
    c8 = R.c8_pack(a, Mp, lane_fill=SENT_F, row_fill=SENT_F)

    def call():
        cb, yb = Buf(c8), Buf(_sent(M, N))
        _ok(_dbg().mpn_debug_c8_rows_to_rowmajor(*cb.a, Mp, M, N, *yb.a))
        cb.read()
        return (yb.read(),)
    assert _same(twice(call)[0], a)


@pytest.mark.parametrize("Cin,Cout", [(3, 5), (8, 128), (12, 130)])
def test_conv_sgd_and_unpack_conv_weights(dev, Cin, Cout):
    rng = np.random.default_rng([Cin, Cout, 4])
    valid = R.conv_valid(Cin, Cout)
    nv = int(valid.sum())
    dw = _sent(*valid.shape)  # the gradient's pad lanes: never read
    dw[valid] = R.draw(rng, nv)
    for fill in (F32(0.0), SENT_F):
        w0, v0 = np.full(valid.shape, fill, F32), np.full(valid.shape, fill, F32)
        w0[valid], v0[valid] = R.draw(rng, nv), R.draw(rng, nv)
        for lr, mom, wd in SGD_PARAMS:
            def call():
                wb, vb, db = Buf(w0), Buf(v0), Buf(dw)
                _ok(_dbg().mpn_debug_conv_sgd(*wb.a, *vb.a, *db.a, Cin, Cout, lr, mom, wd))
                db.read()
                return wb.read(), vb.read()
            w1, v1 = twice(call)
            ew, ev = R.sgd_f32(w0, v0, dw, lr, mom, wd)
            assert _same(w1[valid], ew[valid]) and _same(v1[valid], ev[valid]), (lr, mom, wd)
            assert _same(w1[~valid], w0[~valid]) and _same(v1[~valid], v0[~valid]), "a pad lane of the conv pack was written"
    # unpack_conv_weights: the inverse of the NumPy `wpk` layout, pad lanes (NaN here) skipped; either output may be null
    w, b = R.draw(rng, (Cout, Cin, 3, 3), zero_frac=0.0), R.draw(rng, Cout, zero_frac=0.0)
    src, bsrc = R.conv_pack(w, fill=SENT_F), np.concatenate([b, _sent(R.conv_coutp(Cout) - Cout)])
    assert _same(R.conv_unpack(src, Cin, Cout), w)
    for want_w, want_b in ((1, 1), (1, 0), (0, 1)):
        def call():
            pb, bb, wo, bo = Buf(src), Buf(bsrc), Buf(_sent(Cout, Cin, 3, 3)), Buf(_sent(Cout))
            _ok(_dbg().mpn_debug_unpack_conv_weights(*pb.a, *bb.a, Cin, Cout, *(wo.a if want_w else NULL), *(bo.a if want_b else NULL)))
            pb.read(), bb.read()
            return wo.read(), bo.read()
        wo, bo = twice(call)
        assert _same(wo, w) if want_w else _is_sent(wo)
        assert _same(bo, b) if want_b else _is_sent(bo)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_vec_sgd(dev, n):
    rng = np.random.default_rng(n)
    b0, v0, db = R.draw(rng, n), R.draw(rng, n), R.draw(rng, n)
    for lr, mom, _ in SGD_PARAMS:
        def call():
            bb, vb, gb = Buf(b0), Buf(v0), Buf(db)
            _ok(_dbg().mpn_debug_vec_sgd(*bb.a, *vb.a, *gb.a, n, lr, mom))
            gb.read()
            return bb.read(), vb.read()
        b1, v1 = twice(call)
        eb, ev = R.sgd_bias_f32(b0, v0, db, lr, mom)
        assert _same(b1, eb) and _same(v1, ev), (n, lr, mom)


@pytest.mark.parametrize("C_,H,W", [(3, 1, 1), (8, 5, 7), (12, 9, 3)])
def test_relu_mask_c8p(dev, C_, H, W):
    rng = np.random.default_rng([C_, H, W])
    x = R.draw(rng, (C_, H, W), zero_frac=0.0)
    pick = rng.integers(0, 8, x.shape)
    for v, val in enumerate((0.0, -0.0, np.nan, 2.0 ** -126)):
        x[pick == v] = val
    n_sp = min(4, x.size)
    x.reshape(-1)[:n_sp] = (0.0, -0.0, np.nan, 2.0 ** -126)[-n_sp:]  # every special value is present wherever the map has room
    gv = R.draw(rng, (C_, H, W), zero_frac=0.0)
    inner = R.c8p_interior(C_, H, W)
    xm, gm = R.c8p_pack(x, fill=SENT_F), R.c8p_pack(gv, fill=SENT_F)
    xm[inner & (R.bits(xm) == SENT)] = 0  # the pad channels of a real map are zero
    exp = gm.copy()
    with np.errstate(invalid="ignore"):
        exp[inner & ~(xm > 0)] = 0

    def call():
        gb, xb = Buf(gm), Buf(xm)
        _ok(_dbg().mpn_debug_relu_mask_c8p(*gb.a, *xb.a, C_, H, W))
        xb.read()
        return (gb.read(),)
    got = twice(call)[0]
    assert _same(got[inner], exp[inner]), "the interior is not g where x > 0, else +0.0"
    assert _is_sent(got[~inner]), "the halo or the pitch padding of g was written"
    with np.errstate(invalid="ignore"):
        tiny = inner & (xm == F32(2.0 ** -126))
    assert tiny.any() and (R.bits(got[tiny]) != 0).all(), "2^-126 > 0: the gradient passes"


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    lib = _dbg()
    B, N, K, Mp = 5, 9, 16, 128
    g, x = Buf(_sent(2, Mp, 8)), Buf(_sent(R.k64(K) // 8, Mp, 8))
    pk, pv = Buf(_sent(R.k64(K) // 8, 128, 8)), Buf(_sent(R.k64(K) // 8, 128, 8))
    bb, vb = Buf(_sent(128)), Buf(_sent(128))
    act, dx = Buf(_sent(2, Mp, 8)), Buf(_sent(2, Mp, 8))
    C_, Kc = 3, 2
    head, rois, gt, lab = Buf(_sent(B, (Kc + 4) * C_)), Buf(_sent(B, 4)), Buf(_sent(B, 4)), Buf(np.zeros(B, np.int32))
    gl, loss = Buf(_sent(R.cdiv((Kc + 4) * C_, 8), Mp, 8)), Buf(_sent(2))
    m4, s4 = (C.c_float * 4)(*R.MEAN4), (C.c_float * 4)(*R.STD4)
    wrm, brm = Buf(_sent(N, K)), Buf(_sent(N))
    Cin, Cout = 3, 5
    cw, cv, cd = (Buf(_sent(*R.conv_valid(Cin, Cout).shape)) for _ in range(3))
    cwo, cbo = Buf(_sent(Cout, Cin, 3, 3)), Buf(_sent(Cout))
    ma, mb = Buf(_sent(*R.c8p_interior(3, 2, 2).shape)), Buf(_sent(*R.c8p_interior(3, 2, 2).shape))
    yrm = Buf(_sent(B, N))

    def loss_call(hd=head.a, B_=B, k=0, Mp_=Mp, g_=gl.a, l_=loss.a, r_=rois.a, lb_=lab.a):
        return lib.mpn_debug_train_loss(*hd, B_, C_, Kc, k, *r_, *gt.a, *lb_, m4, s4, 1, BW, *g_, Mp_, *l_)

    def wgrad(g_=g.a, x_=x.a, w_=pk.a, v_=pv.a, B_=B, gMp=Mp, xMp=Mp, inner=1):
        return lib.mpn_debug_sgd_wgrad_c8(*g_, gMp, *x_, xMp, B_, N, K, inner, *w_, *v_, 0.1, 0.9, 0.0)

    def bias(g_=g.a, b_=bb.a, v_=vb.a, B_=B, gMp=Mp):
        return lib.mpn_debug_sgd_bias_c8(*g_, gMp, B_, N, *b_, *v_, 0.1, 0.9)

    def dgrad(g_=g.a, w_=pk.a, a_=act.a, d_=dx.a, B_=B, gMp=Mp, xMp=Mp):
        return lib.mpn_debug_linear_dgrad_c8(*g_, gMp, B_, N, *w_, K, *a_, *d_, xMp, 1.0)

    def drop(y_=g.a, B_=B, Mp_=Mp):
        return lib.mpn_debug_dropout_c8(*y_, Mp_, B_, N, 0, 1, 2, 0, 0, 1.0)

    def torm(c_=g.a, y_=yrm.a, M_=B, Mp_=Mp):
        return lib.mpn_debug_c8_rows_to_rowmajor(*c_, Mp_, M_, N, *y_)

    def pack(w_=wrm.a, b_=brm.a, p_=pk.a, bp_=bb.a, inner=1, K_=K):
        return lib.mpn_debug_pack_linear_weights(*w_, *b_, K_, N, inner, *p_, *bp_)

    def unpack(p_=pk.a, bp_=bb.a, w_=wrm.a, b_=brm.a, n0=0, n1=N, inner=1):
        return lib.mpn_debug_unpack_linear_weights(*p_, *bp_, K, N, inner, n0, n1, *w_, *b_)

    def csgd(w_=cw.a, v_=cv.a, d_=cd.a, Cin_=Cin):
        return lib.mpn_debug_conv_sgd(*w_, *v_, *d_, Cin_, Cout, 0.1, 0.9, 0.0)

    def vsgd(b_=bb.a, v_=vb.a, d_=brm.a, n=N):
        return lib.mpn_debug_vec_sgd(*b_, *v_, *d_, n, 0.1, 0.9)

    def relu(g_=ma.a, x_=mb.a, C2=3):
        return lib.mpn_debug_relu_mask_c8p(*g_, *x_, C2, 2, 2)

    def cunpack(p_=cw.a, b_=bb.a, w_=cwo.a, bo_=cbo.a, Cout_=Cout):
        return lib.mpn_debug_unpack_conv_weights(*p_, *b_, Cin, Cout_, *w_, *bo_)

    refused = [
        # a short buffer, one per buffer of every entry
        (loss_call, dict(hd=head.short())), (loss_call, dict(g_=gl.short())), (loss_call, dict(l_=loss.short())), (loss_call, dict(r_=rois.short())),
        (loss_call, dict(lb_=lab.short())),
        (wgrad, dict(g_=g.short())), (wgrad, dict(x_=x.short())), (wgrad, dict(w_=pk.short())), (wgrad, dict(v_=pv.short())),
        (bias, dict(g_=g.short())), (bias, dict(b_=(bb.a[0], N - 1))), (bias, dict(v_=(vb.a[0], N - 1))),
        (dgrad, dict(g_=g.short())), (dgrad, dict(w_=pk.short())), (dgrad, dict(a_=act.short())), (dgrad, dict(d_=dx.short())),
        (drop, dict(y_=g.short())), (torm, dict(c_=g.short())), (torm, dict(y_=yrm.short())),
        (pack, dict(w_=wrm.short())), (pack, dict(b_=brm.short())), (pack, dict(p_=pk.short())), (pack, dict(bp_=bb.short())),
        (unpack, dict(p_=pk.short())), (unpack, dict(bp_=bb.short())), (unpack, dict(w_=wrm.short())), (unpack, dict(b_=brm.short())),
        (csgd, dict(w_=cw.short())), (csgd, dict(v_=cv.short())), (csgd, dict(d_=cd.short())),
        (vsgd, dict(b_=(bb.a[0], N - 1))), (vsgd, dict(v_=(vb.a[0], N - 1))), (vsgd, dict(d_=brm.short())),
        (relu, dict(g_=ma.short())), (relu, dict(x_=mb.short())),
        (cunpack, dict(p_=cw.short())), (cunpack, dict(w_=cwo.short())), (cunpack, dict(bo_=cbo.short())), (cunpack, dict(b_=(bb.a[0], Cout - 1))),
    ]
    for fn, kw in refused:
        assert fn(**kw) == MPN_EINVAL and "footprint" in _err(), (fn.__name__, kw, _err())
    bad_args = [
        # B <= 0 and Mp < B, wherever an entry has them
        (loss_call, dict(B_=0)), (loss_call, dict(B_=-1)), (loss_call, dict(Mp_=B - 1)), (loss_call, dict(k=Kc)), (loss_call, dict(k=-1)),
        (wgrad, dict(B_=0)), (wgrad, dict(B_=-2)), (wgrad, dict(gMp=B - 1)), (wgrad, dict(xMp=B - 1)), (wgrad, dict(inner=0)), (wgrad, dict(inner=3)),
        (bias, dict(B_=0)), (bias, dict(gMp=B - 1)),
        (dgrad, dict(B_=0)), (dgrad, dict(gMp=B - 1)), (dgrad, dict(xMp=B - 1)),
        (drop, dict(B_=0)), (drop, dict(Mp_=B - 1)),
        (torm, dict(M_=0)), (torm, dict(Mp_=B - 1)),
        (pack, dict(inner=3)), (pack, dict(K_=0)), (unpack, dict(inner=3)), (unpack, dict(n0=2, n1=2)), (unpack, dict(n1=N + 1)), (unpack, dict(n0=-1)),
        (csgd, dict(Cin_=0)), (vsgd, dict(n=0)), (relu, dict(C2=0)), (cunpack, dict(Cout_=0)),
    ]
    for fn, kw in bad_args:
        assert fn(**kw) == MPN_EINVAL and "invalid argument" in _err(), (fn.__name__, kw, _err())
    for buf in (g, x, pk, pv, bb, vb, act, dx, head, rois, gt, gl, loss, wrm, brm, cw, cv, cd, cwo, cbo, ma, mb, yrm):
        assert _is_sent(buf.read()), "a refused call wrote something"
    # the handle-free library state stays usable
    b0 = R.draw(np.random.default_rng(0), 7)
    b1, v1, d1 = Buf(b0), Buf(b0), Buf(b0)
    _ok(lib.mpn_debug_vec_sgd(*b1.a, *v1.a, *d1.a, 7, 0.5, 0.5))
    eb, ev = R.sgd_bias_f32(b0, b0, b0, 0.5, 0.5)
    assert _same(b1.read(), eb) and _same(v1.read(), ev)
