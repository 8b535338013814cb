"""The conv-block half of multipathnet_amd/csrc/train.hip, one launch at a time, against float64 and against NumPy restatements of the orders
train.h documents: roi_pool_backward_kernel (both operand layouts, windows on and off), conv3x3_wgrad_kernel + conv_wgrad_reduce_kernel,
conv_bias_grad_kernel, maxpool2x2_backward_kernel<8>, pack_conv_w_dgrad_kernel, scale_momentum_kernel, the segmented mix-layer forms
(seg_wgrad_kernel, seg_wgrad_sgd_kernel, seg_bias_sgd_kernel) and the split loss.  Until now they were reached only through whole training
steps on two small networks and through the three public NCHW entries, which run other forms than the trainer's.

The kernels are called through the mpn_debug_* pass-throughs of train_debug.hip (debug flavour only): raw device pointers in the kernels' own
layouts, the product's host wrappers, an element count per buffer.  Layouts, orders, references and input sets are
tests/train_conv_kernels_np.py's, checked on the CPU in tests/test_train_conv_kernels_ref_cpu.py, which also shows that a sequential fp32
evaluation of every input set used here meets the bounds.  DESIGN.md section 13.14.

Common setup (tests/test_gpu_train_kernels_numerics.py's Buf): every device buffer sits between two guard zones of 256 sentinel NaNs
(0x7FA5A5A5).  What the contract says is not written holds the sentinel and must keep its bits (map halos and pitch padding, the records of
pad couts in `part`, the pad lanes of a C8P destination of the ROI sum, rows >= B); pad lanes it says are written +0.0 must be exactly +0.0.
What it says is not read holds NaN: G's halo and, for the weight gradient, the pad channels of its last block; rows outside [n0, n1) of g
and rois (their arg-max points at cell 0, so a row read by mistake would carry its NaN into the sum); X's halo for the pool backward, the
cells outside the map in a last odd row or column among them; rows >= B and lanes >= N of the segmented operands; stale `part`.  X's halo
for conv3x3_wgrad is zero: it is the padding.  Real values have magnitudes in [2^-6, 2^3] plus exact zeros.  Every case runs twice on fresh
buffers: the same bits.  Every comparison prints an ACC line.

Tiers.
  bit-exact   the ROI sum equals the fp32 ordered sum, windows = 1 equals windows = 0; the pool backward equals the routing; dw equals the
              emulated reduce of the `part` slabs read back from the same call (groups of 8 ascending, group sums ascending, then
              f32(dw_old + v)); conv_bias_grad and the two segmented second stages equal their emulated orders; wpk_t and zero_b equal the
              layout restatement and wino_t the forward Winograd packer's output for W'; scale_momentum is f32(v * f); train_loss_split
              gives train_loss's bits.
  exact       integer operands in [-2, 2]: every partial sum is an integer below 2^24, so `part`, dw, db and the three outputs of the
              public mpn_conv3x3_backward (B = 2) equal float64 bit for bit — a dropped or doubled pixel, a shifted tap or a segment
              boundary off by one shows without any tolerance.
  derived     |r - r64| <= (n + 1) * 2^-23 * sum |a| |b|: n = the segment's pixels for a `part` slab, H * W * images + images for dw and
              db, nseg * B + nseg for the segmented dW and db.

What the module found.  No kernel computes a wrong value.  One sentence was wrong: conv_wgrad_reduce_kernel's comment said the pad-cin
lanes of `part` are never written by conv3x3_wgrad_kernel.  The kernel stores whole 32-byte records, so the pad-cin lanes of every written
record (cout < Cout) receive the sums over X's pad channels, +0.0 for a real map; only the records of pad couts are left alone.  The reduce
masks both, so dw was always right.  The sentence is corrected in train.hip and stated in train.h, and test_conv3x3_wgrad asserts the +0.0
(and, with NaN in X's pad channels, that dw's pad lanes are still +0.0 and its other lanes keep their bits).  The issue's footprint of
the trainer-layout gradient matrix, ceil(C * PP / 8) records, is too small when C is no multiple of 8: the layout has ceil(C / 8) * PP
records, and mpn_debug_roi_pool_backward asks for those.

MEASURED on the MI355X (largest observed error / bound per family, from the ACC lines; DESIGN.md section 13.14 has the same table):
  conv3x3_wgrad part slabs   0.248 (8 -> 40, 19 x 27, the one-pixel second segment: the product's rounding alone; <= 0.033 on 512-pixel
                             segments), 78 comparisons                                             (sequential fp32 on the CPU: 0.248)
  conv3x3_wgrad dw           0.128 (24 -> 129, 2 x 9); 0.007 and below from 512 pixels on, 22 comparisons              (CPU: 0.128)
  conv_bias_grad db          0.081 (7 channels, 1 x 2), 30 comparisons, bits = the emulated order's   (CPU: 0.058 sequential, 0.081 its order)
  segmented dW               0.105 (nseg 1, N 1, K 8, B 1), 11 cases                                                    (CPU: 0.105)
  segmented db               0.015 (nseg 8, N 7, B 2), 11 cases, bits = the emulated order's          (CPU: 0.012 sequential, 0.015 its order)
  ROI sum, synthetic arg-max 0.185 (2 x 33 bins, C 12, B 3), 3 cases; bit-equal to the ordered fp32 sum                            (CPU: 0.185)
  745 bit-exact comparisons, none differing; two runs in a row print the same ACC lines.  The module's wall time is 5.3 s (100 tests).

Mutations tried on scratch copies of the debug library (MI355X; each only drops work or changes arithmetic, every access in bounds), with
the tests that fail on each:
  conv3x3_wgrad_kernel's segment end as p1 - 1; its tap as (tap + 1) mod 9      test_conv3x3_wgrad (all 11), test_public_conv3x3_backward_exact (all 11)
  conv_wgrad_reduce_kernel with groups of 7                                     test_conv3x3_wgrad at 17 x 241 and 91 x 91 (8 + 1 slabs are still one chain)
  conv_wgrad_reduce_kernel without its ci < Cin mask                            test_conv3x3_wgrad, the four shapes with Cin % 8 != 0
  roi_pool_backward_kernel: 1u << (ph & 15)                                     test_roi_pool_backward, the four 32 x 32 poolings
    x > ws in the window test / rows descending                                 test_roi_pool_backward (20 / 23 cases)
    roundf -> rintf in its copy of roi_bin_bounds, rule 0 / rule 1              test_roi_pool_backward (10 / 9 cases of that rule)
    the batch clamp's upper arm to map 0 / the - 1 dropped                      test_roi_pool_backward, the six B = 3 cases
  maxpool2x2_backward_kernel: >= in the scan / in the ReLU mask                 test_maxpool2x2_backward_c8p (8 / 4 cases)
    its pad-lane guard removed                                                  test_maxpool2x2_backward_c8p — only since X's pad channels hold a positive value
  conv_bias_grad_kernel's tree from 8                                           test_conv_bias_grad (19)
  seg_wgrad_sgd_kernel with groups of 7 / seg_bias_sgd_kernel's leaf tree from 16   test_segmented_forms from nseg 9 / from nseg 49 on
  seg_wgrad_kernel's last row dropped                                           test_segmented_forms (all 11)
  pack_conv_w_dgrad_kernel without the flip in wpk_t / in the Torch-layout W'   test_pack_conv_weights_dgrad (all 6), test_public_conv3x3_backward_exact
  scale_momentum_kernel's tail one short / its loop cut to one trip             test_scale_momentum — every n with a tail only since the special values
                                                                                keep out of the last four floats / the largest n
  train_loss_kernel<true>'s last box chunk dropped                              test_train_loss_split (all 3)
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_train_kernels_numerics as T  # noqa: E402  (Buf, twice, _acc and the sentinel helpers: one setup for both modules)
import train_conv_kernels_np as K  # noqa: E402
import train_kernels_np as R  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENT, SENT_F = R.SENT, R.SENT_F
MPN_EINVAL = -1
Buf, twice, NULL = T.Buf, T.twice, T.NULL
_sent, _same, _same_nanpos = T._sent, T._same, T._same_nanpos
cf, ci, cs, vp = C.c_float, C.c_int, C.c_size_t, C.c_void_p
BW = 1.5
WORST = {}


@functools.lru_cache(maxsize=None)
def _dbg():
    lib = T._dbg()
    b = [vp, cs]
    f4 = C.POINTER(C.c_float * 4)
    lib.mpn_debug_train_loss_split.argtypes = b + b + [ci, ci, ci, ci] + b + b + b + [f4, f4, ci, cf] + b + b + [ci] + b
    lib.mpn_debug_scale_momentum.argtypes = b + [cs, cf]
    lib.mpn_debug_roi_pool_backward.argtypes = b + b + b + [ci] * 13 + [cf, ci] + b
    lib.mpn_debug_conv3x3_wgrad.argtypes = b + b + [ci] * 4 + b + b + [ci]
    lib.mpn_debug_conv_bias_grad.argtypes = b + [ci] * 3 + b + [ci]
    lib.mpn_debug_maxpool2x2_backward_c8p.argtypes = b + b + b + [ci] * 4
    lib.mpn_debug_pack_conv_weights_dgrad.argtypes = b + [ci, ci] + b + b + b + b
    lib.mpn_debug_pack_conv_weights_wino.argtypes = b + [ci, ci] + b
    lib.mpn_debug_roi_pool_form.argtypes = [ci] + b + [ci, ci, ci, ci, cs] + b + [ci, ci, ci, ci, cf, ci, ci, ci, cf] + b + b + b
    lib.mpn_debug_sgd_wgrad_seg_c8.argtypes = b + b + [ci] * 5 + b + b + b + [cf, cf, cf]
    lib.mpn_debug_sgd_bias_seg_c8.argtypes = b + [ci] * 4 + b + b + [cf, cf]
    lib.mpn_conv3x3_backward_workspace_bytes.restype = cs
    lib.mpn_conv3x3_backward_workspace_bytes.argtypes = [ci] * 5
    lib.mpn_conv3x3_backward.argtypes = [vp, ci, ci, ci, ci, vp, vp, ci, vp, vp, vp, vp, cs, vp]
    return lib


def _err():
    return _dbg().mpn_last_error().decode()


def _ok(rc):
    assert rc == 0, (rc, _err())


def _acc(family, tag, err, bound):
    r = T._acc(family + " " + tag, np.asarray(err), np.asarray(bound))
    WORST[family] = max(WORST.get(family, 0.0), r)
    print("ACC-MAX %-40s %.3f" % (family, WORST[family]))
    return r


def _bits_acc(tag, got, ref, nanpos=False):
    """a bit-exact comparison, with its ACC line"""
    got, ref = np.asarray(got, F32), np.asarray(ref, F32)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    bad = int((R.bits(got) != R.bits(ref)).sum()) if not nanpos else (0 if _same_nanpos(got, ref) else -1)
    print("ACC %-60s bits differ in %d of %d" % (tag, bad, got.size))
    assert bad == 0, tag


def _is_sent(a):
    """every 32-bit word still holds the sentinel (float or int32 buffers)"""
    return bool((np.ascontiguousarray(a).view(np.uint32) == SENT).all())


def _sent_i(*shape):
    return np.full(shape, SENT, np.uint32).view(np.int32)


# ---- conv3x3_wgrad ---------------------------------------------------------------------------------------------------------------------------
def _run_wgrad(xm, gm, part0, dw0, Cin, Cout, H, W, accumulate):
    def call():
        xb, gb, pb, db = Buf(xm), Buf(gm), Buf(part0), Buf(dw0)
        _ok(_dbg().mpn_debug_conv3x3_wgrad(*xb.a, *gb.a, Cin, Cout, H, W, *pb.a, *db.a, accumulate))
        part, dw = pb.read(), db.read()
        assert _same(xb.read(), xm) and _same(gb.read(), gm), "an input was written"
        return part, dw
    return twice(call)


@pytest.mark.parametrize("shape", K.WGRAD_SHAPES, ids=["%dto%d_%dx%d" % s for s in K.WGRAD_SHAPES])
def test_conv3x3_wgrad(dev, shape):
    Cin, Cout, H, W = shape
    nseg, valid = K.n_segments(H, W), K.conv_valid(Cin, Cout)
    written = np.zeros(valid.shape, bool)
    written[:, :, :Cout, :] = True   # whole records of the real couts
    tag = "%dto%d %dx%d" % shape
    for exact in (False, True):
        imgs = K.wgrad_inputs(*shape, exact=exact)
        tot64, tot_mag, dw_prev = 0.0, 0.0, None
        for i, (x, g) in enumerate(imgs):
            xm = K.c8p_pack(x, pad=0.0, halo=0.0, pitch=SENT_F)          # the halo is the padding; nothing beyond it is read
            gm = K.c8p_pack(g, pad=SENT_F, halo=SENT_F, pitch=SENT_F)    # G's halo and pad channels: never read
            part0 = _sent(nseg, *valid.shape)                            # stale partial sums: NaN
            if dw_prev is None:
                dw0 = _sent(*valid.shape)
            else:
                dw0 = np.where(valid, dw_prev, SENT_F).astype(F32)       # the running gradient; stale pad lanes must come out +0.0
            part, dw = _run_wgrad(xm, gm, part0, dw0, Cin, Cout, H, W, int(i > 0))
            s64, mag, npx = K.wgrad_slabs64(x, g)
            assert _is_sent(part[:, ~written]), "a record of a pad cout of `part` was written"
            assert (R.bits(part[:, written & ~valid]) == 0).all(), "the pad-cin lanes of a written record are not +0.0 (X's pad channels are zero)"
            got = K.slabs_unpack(part, Cin, Cout)
            assert np.isfinite(got).all()
            if exact:
                _bits_acc("wgrad part exact %s img %d" % (tag, i), got, s64.astype(F32))
            else:
                for s in range(nseg):
                    _acc("conv3x3_wgrad part", "%s seg %d img %d" % (tag, s, i), np.abs(got[s].astype(F64) - s64[s]), (npx[s] + 1) * K.U23 * mag[s])
            # dw is the documented reduce of these very slabs
            emu = K.wgrad_reduce_f32(part, Cin, Cout, dw0 if i > 0 else None)
            _bits_acc("wgrad dw = reduce(part) %s img %d acc %d" % (tag, i, int(i > 0)), dw, emu)
            assert (R.bits(dw[~valid]) == 0).all(), "a pad lane of dw is not +0.0"
            tot64, tot_mag = tot64 + s64.sum(0), tot_mag + mag.sum(0)
            n = H * W * (i + 1) + (i + 1)
            dwv = K.conv_unpack(dw, Cin, Cout)
            if exact:
                _bits_acc("wgrad dw exact %s img %d" % (tag, i), dwv, tot64.astype(F32))
            else:
                _acc("conv3x3_wgrad dw", "%s images %d" % (tag, i + 1), np.abs(dwv.astype(F64) - tot64), (n + 1) * K.U23 * tot_mag)
            if i == 0 and Cin % 8 and not exact:
                # NaN in X's pad channels: masked by the reduce — dw's pad lanes are +0.0 and every other lane keeps its bits
                xn = K.c8p_pack(x, pad=SENT_F, halo=0.0, pitch=SENT_F)
                _, dwn = _run_wgrad(xn, gm, part0, dw0, Cin, Cout, H, W, 0)
                _bits_acc("wgrad dw with NaN pad cins %s" % tag, dwn, dw)
            dw_prev = dw


# ---- conv_bias_grad --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cout,H,W", K.bias_maps(), ids=["%d_%dx%d" % m for m in K.bias_maps()])
def test_conv_bias_grad(dev, Cout, H, W):
    tag = "%d %dx%d" % (Cout, H, W)
    for exact in (False, True):
        tot64, mag, db_prev = np.zeros(Cout), np.zeros(Cout), None
        for i, g in enumerate(K.bias_inputs(Cout, H, W, exact)):
            gm = K.c8p_pack(g, pad=SENT_F, halo=SENT_F, pitch=SENT_F)   # pad channels: read into lanes nothing is stored from
            db0 = _sent(Cout) if db_prev is None else db_prev

            def call():
                gb, db = Buf(gm), Buf(db0)
                _ok(_dbg().mpn_debug_conv_bias_grad(*gb.a, Cout, H, W, *db.a, int(i > 0)))
                assert _same(gb.read(), gm)
                return (db.read(),)
            db = twice(call)[0]
            _bits_acc("bias_grad order %s img %d" % (tag, i), db, K.bias_grad_f32(g, db_prev))
            tot64, mag = tot64 + g.astype(F64).sum((1, 2)), mag + np.abs(g.astype(F64)).sum((1, 2))
            if exact:
                _bits_acc("bias_grad exact %s img %d" % (tag, i), db, tot64.astype(F32))
            else:
                _acc("conv_bias_grad db", "%s images %d" % (tag, i + 1), np.abs(db.astype(F64) - tot64), (H * W * (i + 1) + (i + 1) + 1) * K.U23 * mag)
            db_prev = db


# ---- the public mpn_conv3x3_backward on integer operands -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", K.WGRAD_SHAPES, ids=["%dto%d_%dx%d" % s for s in K.WGRAD_SHAPES])
def test_public_conv3x3_backward_exact(dev, shape):
    Cin, Cout, H, W = shape
    lib = _dbg()
    rng = np.random.default_rng([Cin, Cout, H, W, 31])
    imgs = K.wgrad_inputs(*shape, exact=True)
    x, g = np.stack([a for a, _ in imgs]), np.stack([b for _, b in imgs])
    w = rng.integers(-2, 3, (Cout, Cin, 3, 3)).astype(F32)
    xt, wt = torch.tensor(x.astype(F64), requires_grad=True), torch.tensor(w.astype(F64), requires_grad=True)
    bt = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(xt, wt, bt, padding=1).backward(torch.tensor(g.astype(F64)))
    ref = [t.grad.numpy() for t in (xt, wt, bt)]
    assert all((np.abs(r) < 2.0 ** 24).all() and (r == np.round(r)).all() for r in ref)
    need = lib.mpn_conv3x3_backward_workspace_bytes(2, Cin, H, W, Cout)

    def call():
        xb, wb, gb = Buf(x), Buf(w), Buf(g)
        gi, gw, gbias = Buf(_sent(2, Cin, H, W)), Buf(_sent(Cout, Cin, 3, 3)), Buf(_sent(Cout))
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)   # every halo and pad lane of the workspace starts as NaN
        _ok(lib.mpn_conv3x3_backward(xb.a[0], 2, Cin, H, W, wb.a[0], gb.a[0], Cout, gi.a[0], gw.a[0], gbias.a[0], vp(ws.data_ptr()), need, None))
        torch.cuda.synchronize()
        return gi.read(), gw.read(), gbias.read()
    out = twice(call)
    for name, got, r in zip(("grad_in", "grad_w", "grad_b"), out, ref):
        _bits_acc("mpn_conv3x3_backward exact %dto%d %dx%d %s" % (shape + (name,)), got, r.astype(F32))


# ---- roi_pool_backward -----------------------------------------------------------------------------------------------------------------------
ROI_MP = 128


def _forward_argmax(feat, rois, C_, H, W, PH, PW, rule, rows):
    """the product's forward (roi_pool_c8, form 0) at the same scale and bin rule, map by map -> arg-max [N, C, PP] int32"""
    N, PP = len(rois), PH * PW
    am = np.zeros((N, C_, PP), np.int32)
    for b in range(feat.shape[0]):
        fb, rb = Buf(K.c8p_pack(feat[b], pad=0.0, halo=F32(2.0 ** 100), pitch=F32(2.0 ** 100))), Buf(rois.reshape(-1))
        xb, ab = Buf(_sent(K.cdiv(C_, 8) * PP * ROI_MP * 8)), Buf(_sent_i(N * C_ * PP))
        _ok(_dbg().mpn_debug_roi_pool_form(0, *fb.a, C_, H, W, 0, 0, *rb.a, 5, N, PH, PW, K.ROI_SCALE, rule, ROI_MP, 0, 1.0, *xb.a, *ab.a, *NULL))
        got = ab.read().reshape(N, C_, PP)
        am[rows == b] = got[rows == b]
    return am


def _run_roi(layout, g, am, rois, by_batch, n0, n1, nb, C_, H, W, PH, PW, windows, rule):
    """-> the sum as [nb, C, H, W], after checking everything the launch must leave alone"""
    N = len(rois)
    gq, aq, rq = g.copy(), am.copy(), rois.copy()
    out_rows = np.ones(N, bool)
    out_rows[n0:n1] = False
    gq[out_rows], aq[out_rows], rq[out_rows] = np.nan, 0, np.nan   # rows outside [n0, n1): never read
    if not by_batch:
        rq[:, 0] = np.nan                                        # the batch column is read by by_batch alone
    if layout == 0:
        gin, out0 = gq, _sent(nb, C_, H, W)
    else:
        gin = K.roi_g_c8(gq, ROI_MP, fill=SENT_F)                # lanes c >= C and rows >= N: never read
        out0 = _sent(*K.c8p_masks(C_, H, W)[0].shape)

    def call():
        gb, ab, rb, ob = Buf(gin), Buf(aq), Buf(rq), Buf(out0)
        _ok(_dbg().mpn_debug_roi_pool_backward(*gb.a, *ab.a, *rb.a, N, layout, ROI_MP, int(by_batch), n0, n1, nb, C_, H, W, PH, PW, windows, K.ROI_SCALE,
                                               rule, *ob.a))
        o = ob.read()
        gb.read(), ab.read(), rb.read()
        return (o,)
    o = twice(call)[0]
    if layout == 0:
        return o
    real, pad, outside = K.c8p_masks(C_, H, W)
    assert _is_sent(o[pad]) and _is_sent(o[outside]), "a pad lane, the halo or the pitch padding of the C8P destination was written"
    return K.c8p_unpack(o, C_, H, W)[None]


@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("case", K.ROI_CASES, ids=["C%d_%dx%d_p%dx%d_N%d_B%d" % c for c in K.ROI_CASES])
def test_roi_pool_backward(dev, case, rule):
    C_, H, W, PH, PW, N, B = case
    feat, rois, g = K.roi_inputs(*case)
    nb, by_batch = max(B, 1), B > 0
    rows = K.roi_rows_map(rois, nb)
    am = _forward_argmax(feat, rois, C_, H, W, PH, PW, rule, rows)
    # the window restatement agrees with the forward, and every arg-max lies inside its window: the windowed sum must equal the plain one
    own = np.stack([K.window_argmax(feat[rows[n]], rois[n:n + 1], PH, PW, K.ROI_SCALE, rule)[0] for n in range(N)])
    assert np.array_equal(own, am), "the forward's arg-max differs from roi_bin_bounds' windows restated in NumPy"
    assert K.argmax_in_windows(am, rois, H, W, PH, PW, K.ROI_SCALE, rule)
    ranges = [(0, N), (2, N - 1)] if by_batch else K.roi_row_ranges(N)
    tag = "C%d %dx%d p%dx%d N%d B%d rule %d" % (case + (rule,))
    for n0, n1 in ranges:
        ref = K.roi_backward(g, am, rois, by_batch, n0, n1, nb, C_, H, W, F32)
        if n0 == n1:
            assert (R.bits(ref) == 0).all()
        for layout in ((0, 1) if nb == 1 else (0,)):
            plain = _run_roi(layout, g, am, rois, by_batch, n0, n1, nb, C_, H, W, PH, PW, 0, rule)
            _bits_acc("roi_backward ordered sum %s layout %d rows [%d, %d)" % (tag, layout, n0, n1), plain, ref)
            win = _run_roi(layout, g, am, rois, by_batch, n0, n1, nb, C_, H, W, PH, PW, 1, rule)
            _bits_acc("roi_backward windows 1 == 0 %s layout %d rows [%d, %d)" % (tag, layout, n0, n1), win, plain)


@pytest.mark.parametrize("PH,PW,C_,B", K.ROI_SYNTH_CASES)
def test_roi_pool_backward_synthetic_argmax(dev, PH, PW, C_, B):
    """arg-max values no forward produced (any cell, many collisions, -1): windows = 0 only.  More than 32 bins along a side: windows = 1 is
    refused, windows = 0 accepted."""
    H, W, N = K.ROI_SYNTH_MAP
    am, g, rois = K.roi_synth_inputs(PH, PW, C_, B)
    ref = K.roi_backward(g, am, rois, True, 0, N, B, C_, H, W, F32)
    got = _run_roi(0, g, am, rois, True, 0, N, B, C_, H, W, PH, PW, 0, 0)
    _bits_acc("roi_backward synthetic arg-max p%dx%d C%d B%d" % (PH, PW, C_, B), got, ref)
    r64 = K.roi_backward(g, am, rois, True, 0, N, B, C_, H, W, F64)
    cnt = K.roi_backward(np.ones_like(g), am, rois, True, 0, N, B, C_, H, W, F64)
    _acc("roi_pool_backward sum", "p%dx%d C%d B%d" % (PH, PW, C_, B), np.abs(got.astype(F64) - r64),
         (cnt + 1) * K.U23 * K.roi_backward(np.abs(g), am, rois, True, 0, N, B, C_, H, W, F64))
    if max(PH, PW) > 32:
        gb, ab, rb, ob = Buf(g), Buf(am), Buf(rois), Buf(_sent(B, C_, H, W))
        rc = _dbg().mpn_debug_roi_pool_backward(*gb.a, *ab.a, *rb.a, N, 0, ROI_MP, 1, 0, N, B, C_, H, W, PH, PW, 1, K.ROI_SCALE, 0, *ob.a)
        assert rc == MPN_EINVAL and "invalid argument" in _err()
        assert _is_sent(ob.read())


# ---- maxpool2x2_backward_c8p -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu_mask", [0, 1])
@pytest.mark.parametrize("C_,H,W", K.POOL_SHAPES)
def test_maxpool2x2_backward_c8p(dev, C_, H, W, relu_mask):
    x, gy = K.pool_inputs(C_, H, W)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    # X's halo (the cells outside an odd map among it): never read.  Its pad channels hold a positive value and dY's NaN: a pad lane that
    # was routed like a real one would carry the NaN into dX (with NaN in X's pad lanes `v > m` would hide a missing guard)
    xm = K.c8p_pack(x, pad=F32(3.0), halo=SENT_F, pitch=SENT_F)
    ym = K.c8p_pack(gy, pad=SENT_F, halo=SENT_F, pitch=SENT_F)
    real, pad, outside = K.c8p_masks(C_, H, W)

    def call():
        xb, yb, db = Buf(xm), Buf(ym), Buf(_sent(*xm.shape))
        _ok(_dbg().mpn_debug_maxpool2x2_backward_c8p(*xb.a, *yb.a, *db.a, C_, H, W, relu_mask))
        assert _same(xb.read(), xm) and _same(yb.read(), ym)
        return (db.read(),)
    dx = twice(call)[0]
    assert ym.shape == (K.cdiv(C_, 8), K.act_hp(Ho), K.act_wp(Wo), 8)
    _bits_acc("maxpool2x2_backward_c8p C%d %dx%d relu %d" % (C_, H, W, relu_mask), K.c8p_unpack(dx, C_, H, W), K.pool_backward(x, gy, relu_mask))
    assert (R.bits(dx[pad]) == 0).all(), "the pad lanes of the last channel block are not +0.0"
    assert _is_sent(dx[outside]), "the halo or the pitch padding of dX was written"


# ---- pack_conv_weights_dgrad -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cin,Cout", K.DGRAD_PACK_SHAPES)
def test_pack_conv_weights_dgrad(dev, Cin, Cout):
    lib = _dbg()
    w = R.draw(np.random.default_rng([Cin, Cout, 32]), (Cout, Cin, 3, 3), zero_frac=0.0)
    wt = K.dgrad_weights(w)
    wpk_ref, zb_ref = K.dgrad_pack(w)
    n_wino = K.cdiv(Cout, 8) * 16 * K.conv_coutp(Cin) * 8

    def wino_of_wt():
        wb, ob = Buf(wt), Buf(_sent(n_wino))
        _ok(lib.mpn_debug_pack_conv_weights_wino(*wb.a, Cout, Cin, *ob.a))   # the forward's packer on the Cout -> Cin layer
        return (ob.read(),)
    wino_ref = twice(wino_of_wt)[0]
    assert not _is_sent(wino_ref[:1]) and np.isfinite(wino_ref).all()
    for with_wino, with_tmp in ((1, 1), (0, 1), (0, 0)):
        def call():
            wb, tb, pb, zb, nb_ = Buf(w), Buf(_sent(w.size)), Buf(_sent(*wpk_ref.shape)), Buf(_sent(zb_ref.size)), Buf(_sent(n_wino))
            _ok(lib.mpn_debug_pack_conv_weights_dgrad(*wb.a, Cin, Cout, *(tb.a if with_tmp else NULL), *pb.a, *zb.a, *(nb_.a if with_wino else NULL)))
            assert _same(wb.read(), w)
            return tb.read(), pb.read(), zb.read(), nb_.read()
        tmp, wpk_t, zb, wino = twice(call)
        tag = "%dto%d wino %d tmp %d" % (Cin, Cout, with_wino, with_tmp)
        _bits_acc("pack_dgrad wpk_t " + tag, wpk_t, wpk_ref)
        assert (R.bits(wpk_t[~K.conv_valid(Cout, Cin)]) == 0).all() and (R.bits(zb) == 0).all(), "pad lanes of wpk_t or the zero bias are not +0.0"
        if with_wino:
            _bits_acc("pack_dgrad W' (Torch layout) " + tag, tmp, wt.reshape(-1))
            _bits_acc("pack_dgrad wino_t " + tag, wino, wino_ref)
        else:
            assert _is_sent(tmp) and _is_sent(wino), "without wino_t neither it nor the scratch is written"
    wb, pb, zb, nb_ = Buf(w), Buf(_sent(*wpk_ref.shape)), Buf(_sent(zb_ref.size)), Buf(_sent(n_wino))
    assert lib.mpn_debug_pack_conv_weights_dgrad(*wb.a, Cin, Cout, *NULL, *pb.a, *zb.a, *nb_.a) == MPN_EINVAL and "invalid argument" in _err()
    assert _is_sent(pb.read()) and _is_sent(zb.read()) and _is_sent(nb_.read())


# ---- scale_momentum --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", K.SCALE_N)
def test_scale_momentum(dev, n):
    v = K.scale_inputs(n)
    host = np.concatenate([v, _sent(19)])   # the floats behind n: not touched
    for f in K.SCALE_F:
        def call():
            b = Buf(host)
            _ok(_dbg().mpn_debug_scale_momentum(b.a[0], n, n, f))
            return (b.read(),)
        got = twice(call)[0]
        with np.errstate(all="ignore"):
            ref = v * F32(f)
        assert ref.dtype == F32
        _bits_acc("scale_momentum n %d f %g" % (n, f), got[:n], ref, nanpos=True)
        assert _is_sent(got[n:]), "a float behind n was written"
        if f == 1.0:
            assert _same_nanpos(got[:n], v)
        if f == 0.0:
            fin = np.isfinite(v)
            assert (R.bits(got[:n])[fin] == np.where(np.signbit(v[fin]), 0x80000000, 0).astype(np.uint32)).all()
    if n >= 8:   # a pointer that is not 16-byte aligned is refused
        b = Buf(host)
        rc = _dbg().mpn_debug_scale_momentum(vp(b.ptr + 4), n - 1, n - 1, 0.5)
        assert rc == MPN_EINVAL and "invalid argument" in _err()
        assert _same(b.read(), host)
    b = Buf(host)
    assert _dbg().mpn_debug_scale_momentum(b.a[0], n - 1, n, 0.5) == MPN_EINVAL and "footprint" in _err() and "d_v" in _err()
    assert _same(b.read(), host)


# ---- train_loss_split ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,Kc", K.SPLIT_CKK)
def test_train_loss_split(dev, C_, Kc):
    lib = _dbg()
    m4, s4 = (C.c_float * 4)(*R.MEAN4), (C.c_float * 4)(*R.STD4)
    for k in range(Kc):
        for B in K.SPLIT_B:
            for norm in (1, 0):
                head, rois, gt, labels = R.loss_inputs(C_, Kc, k, B)
                cls, box = np.ascontiguousarray(head[:, :Kc * C_]), np.ascontiguousarray(head[:, Kc * C_:])
                Mp = R.round_up(B, 128) + 128
                qc, qb = R.cdiv(Kc * C_, 8), R.cdiv(4 * C_, 8)
                loss, g = T._run_loss(head, rois, gt, labels, B, C_, Kc, k, norm)

                def call():
                    cb, xb, rb, tb, lb = Buf(cls), Buf(box), Buf(rois), Buf(gt), Buf(np.asarray(labels, np.int32))
                    gc, gx, ob = Buf(_sent(qc, Mp, 8)), Buf(_sent(qb, Mp, 8)), Buf(_sent(4))
                    _ok(lib.mpn_debug_train_loss_split(*cb.a, *xb.a, B, C_, Kc, k, *rb.a, *tb.a, *lb.a, m4, s4, norm, BW, *gc.a, *gx.a, Mp, *ob.a))
                    cb.read(), xb.read(), rb.read(), tb.read(), lb.read()
                    return ob.read(), gc.read(), gx.read()
                l2, gc, gx = twice(call)
                assert _is_sent(l2[2:]) and _is_sent(gc[:, B:]) and _is_sent(gx[:, B:]), "rows >= B (or floats behind the two losses) were written"
                fc, fx = gc[:, :B].transpose(1, 0, 2).reshape(B, qc * 8), gx[:, :B].transpose(1, 0, 2).reshape(B, qb * 8)
                assert (R.bits(fc[:, Kc * C_:]) == 0).all() and (R.bits(fx[:, 4 * C_:]) == 0).all(), "pad lanes are not +0.0"
                tag = "C %d K %d k %d B %d norm %d" % (C_, Kc, k, B, norm)
                _bits_acc("train_loss_split losses " + tag, l2[:2], loss)
                _bits_acc("train_loss_split g_cls " + tag, fc[:, :Kc * C_], g[:, :Kc * C_])
                _bits_acc("train_loss_split g_bbox " + tag, fx[:, :4 * C_], g[:, Kc * C_:])


# ---- the segmented forms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.SEG_CASES, ids=["nseg%d_N%d_K%d_B%d_Mp%d" % c for c in K.SEG_CASES])
def test_segmented_forms(dev, case):
    nseg, N, Kk, B, Mp = case
    lib = _dbg()
    g, x = K.seg_inputs(nseg, N, Kk, B)
    nch, NP = R.k64(Kk) // 8, R.lin_np(N)
    g_c8 = K.seg_pack(g, Mp, K.cdiv(N, 8), lane_fill=SENT_F, row_fill=SENT_F)   # lanes >= N and rows >= B of every segment: never used
    x_c8 = K.seg_pack(x, Mp, nch, lane_fill=SENT_F, row_fill=SENT_F)
    valid = R.lin_valid(Kk, N, 1)
    g2, x2 = g.reshape(nseg * B, N), x.reshape(nseg * B, Kk)
    n = nseg * B + nseg
    tag = "nseg %d N %d K %d B %d Mp %d" % case
    rng = np.random.default_rng([nseg, N, Kk, B, 33])
    z = np.where(valid, F32(0), SENT_F).astype(F32)
    w0, v0 = z.copy(), z.copy()
    w0[valid], v0[valid] = R.draw(rng, int(valid.sum())), R.draw(rng, int(valid.sum()))
    dW = None
    for (wa, va), (lr, mom, wd) in (((z, z), (1.0, 0.0, 0.0)), ((w0, v0), (0.25, 0.5, 5e-4)), ((w0, v0), (0.0, 0.9, 5e-4))):
        def call():
            gb, xb, pb, wb, vb = Buf(g_c8), Buf(x_c8), Buf(_sent(nseg, nch, NP, 8)), Buf(wa), Buf(va)
            _ok(lib.mpn_debug_sgd_wgrad_seg_c8(*gb.a, *xb.a, Mp, nseg, B, N, Kk, *pb.a, *wb.a, *vb.a, lr, mom, wd))
            return pb.read(), wb.read(), vb.read()
        part, w1, v1 = twice(call)
        assert np.isfinite(part[:, valid]).all()
        with np.errstate(invalid="ignore"):
            s = K.group_sum_f32(part)   # the slabs in groups of 8 ascending, the group sums ascending
        ew, ev = R.sgd_f32(wa, va, s, lr, mom, wd)
        _bits_acc("seg_wgrad second stage + sgd %s lr %g" % (tag, lr), np.stack([w1[valid], v1[valid]]), np.stack([ew[valid], ev[valid]]))
        assert _is_sent(w1[~valid]) and _is_sent(v1[~valid]), "a pad lane of the packing was touched"
        if dW is None:
            dW = R.lin_unpack(v1, Kk, N, 1)
            _acc("segmented dW", tag, np.abs(dW.astype(F64) - g2.astype(F64).T @ x2.astype(F64)), R.dot_bound(g2, x2, n))
        if lr == 0.0:
            assert _same(w1[valid], wa[valid])
    b0, vb0 = _sent(NP), _sent(NP)
    b0[:N], vb0[:N] = R.draw(rng, N), R.draw(rng, N)
    db = K.seg_bias_f32(g)
    ref, bound = g2.astype(F64).sum(0), (n + 1) * K.U23 * np.abs(g2.astype(F64)).sum(0)
    for lr, mom in ((1.0, 0.0), (1e-3, 0.9)):
        def call():
            gb, bb, vb = Buf(g_c8), Buf(b0), Buf(vb0)
            _ok(lib.mpn_debug_sgd_bias_seg_c8(*gb.a, Mp, nseg, B, N, *bb.a, *vb.a, lr, mom))
            return bb.read(), vb.read()
        b1, v1 = twice(call)
        eb, ev = R.sgd_bias_f32(b0[:N], vb0[:N], db, lr, mom)
        _bits_acc("seg_bias second stage + step %s lr %g" % (tag, lr), np.stack([b1[:N], v1[:N]]), np.stack([eb, ev]))
        assert _is_sent(b1[N:]) and _is_sent(v1[N:])
        if mom == 0.0:
            _acc("segmented db", tag, np.abs(v1[:N].astype(F64) - ref), bound)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    """each buffer of each new entry one element short: MPN_EINVAL naming the buffer, nothing launched"""
    lib = _dbg()
    m4, s4 = (C.c_float * 4)(*R.MEAN4), (C.c_float * 4)(*R.STD4)
    Cin, Cout, H, W = 9, 33, 5, 7
    ax, ag = int(np.prod(K.c8p_masks(Cin, H, W)[0].shape)), int(np.prod(K.c8p_masks(Cout, H, W)[0].shape))
    wpk = int(np.prod(K.conv_valid(Cin, Cout).shape))
    xm, gm, part, dw, db = Buf(_sent(ax)), Buf(_sent(ag)), Buf(_sent(wpk)), Buf(_sent(wpk)), Buf(_sent(Cout))
    ay = int(np.prod(K.c8p_masks(Cin, 3, 4)[0].shape))
    px, py, pd = Buf(_sent(ax)), Buf(_sent(ay)), Buf(_sent(ax))
    w, tmp = Buf(_sent(Cout * Cin * 9)), Buf(_sent(Cout * Cin * 9))
    wpk_t, zb = Buf(_sent(K.cdiv(Cout, 8) * 9 * K.conv_coutp(Cin) * 8)), Buf(_sent(K.conv_coutp(Cin)))
    wino_t, wino = Buf(_sent(K.cdiv(Cout, 8) * 16 * K.conv_coutp(Cin) * 8)), Buf(_sent(K.cdiv(Cin, 8) * 16 * K.conv_coutp(Cout) * 8))
    N, C_, PH, PW = 5, 12, 3, 5
    PP = PH * PW
    rg0, rg1 = Buf(_sent(N * C_ * PP)), Buf(_sent(2 * PP * ROI_MP * 8))
    ram, rro = Buf(_sent_i(N * C_ * PP)), Buf(_sent(N * 5))
    ro0, ro1 = Buf(_sent(2 * C_ * H * W)), Buf(_sent(int(np.prod(K.c8p_masks(C_, H, W)[0].shape))))
    B, Cc, Kc, Mp = 5, 3, 2, 128
    cls, box, rois, gt, lab = Buf(_sent(B, Kc * Cc)), Buf(_sent(B, 4 * Cc)), Buf(_sent(B, 4)), Buf(_sent(B, 4)), Buf(np.zeros(B, np.int32))
    gcl, gbx, loss = Buf(_sent(1, Mp, 8)), Buf(_sent(2, Mp, 8)), Buf(_sent(2))

    def wgrad(x_=xm.a, g_=gm.a, p_=part.a, d_=dw.a, H_=H):
        return lib.mpn_debug_conv3x3_wgrad(*x_, *g_, Cin, Cout, H_, W, *p_, *d_, 0)

    def bias(g_=gm.a, d_=db.a, Cout_=Cout):
        return lib.mpn_debug_conv_bias_grad(*g_, Cout_, H, W, *d_, 0)

    def pool(x_=px.a, y_=py.a, d_=pd.a, C2=Cin):
        return lib.mpn_debug_maxpool2x2_backward_c8p(*x_, *y_, *d_, C2, H, W, 1)

    def dpack(w_=w.a, t_=tmp.a, p_=wpk_t.a, z_=zb.a, n_=wino_t.a, Cin_=Cin):
        return lib.mpn_debug_pack_conv_weights_dgrad(*w_, Cin_, Cout, *t_, *p_, *z_, *n_)

    def wpack(w_=w.a, o_=wino.a, Cin_=Cin):
        return lib.mpn_debug_pack_conv_weights_wino(*w_, Cin_, Cout, *o_)

    def roi(layout=0, g_=None, a_=ram.a, r_=rro.a, o_=None, n0=0, n1=N, B_=None, Mp_=ROI_MP, rule=0, PH_=PH):
        g_ = g_ or (rg0.a if layout == 0 else rg1.a)
        o_ = o_ or (ro0.a if layout == 0 else ro1.a)
        B_ = B_ or (2 if layout == 0 else 1)
        return lib.mpn_debug_roi_pool_backward(*g_, *a_, *r_, N, layout, Mp_, 1, n0, n1, B_, C_, H, W, PH_, PW, 0, 0.25, rule, *o_)

    def split(c_=cls.a, x_=box.a, r_=rois.a, t_=gt.a, l_=lab.a, gc_=gcl.a, gx_=gbx.a, o_=loss.a, B_=B, k=0, Mp_=Mp):
        return lib.mpn_debug_train_loss_split(*c_, *x_, B_, Cc, Kc, k, *r_, *t_, *l_, m4, s4, 1, BW, *gc_, *gx_, Mp_, *o_)

    refused = [
        (wgrad, dict(x_=xm.short()), "d_x"), (wgrad, dict(g_=gm.short()), "d_g"), (wgrad, dict(p_=part.short()), "d_part"), (wgrad, dict(d_=dw.short()), "d_dw"),
        (bias, dict(g_=gm.short()), "d_g"), (bias, dict(d_=db.short()), "d_db"),
        (pool, dict(x_=px.short()), "d_x"), (pool, dict(y_=py.short()), "d_dy"), (pool, dict(d_=pd.short()), "d_dx"),
        (dpack, dict(w_=w.short()), "d_w"), (dpack, dict(t_=tmp.short()), "d_tmp"), (dpack, dict(p_=wpk_t.short()), "d_wpk_t"),
        (dpack, dict(z_=zb.short()), "d_zero_b"), (dpack, dict(n_=wino_t.short()), "d_wino_t"),
        (wpack, dict(w_=w.short()), "d_w"), (wpack, dict(o_=wino.short()), "d_wino"),
        (roi, dict(layout=0, g_=rg0.short()), "d_g"), (roi, dict(layout=1, g_=rg1.short()), "d_g"), (roi, dict(a_=ram.short()), "d_argmax"),
        (roi, dict(r_=rro.short()), "d_rois"), (roi, dict(layout=0, o_=ro0.short()), "d_out"), (roi, dict(layout=1, o_=ro1.short()), "d_out"),
        (split, dict(c_=cls.short()), "d_cls"), (split, dict(x_=box.short()), "d_bbox"), (split, dict(r_=rois.short()), "d_rois"),
        (split, dict(t_=gt.short()), "d_gt"), (split, dict(l_=lab.short()), "d_labels"), (split, dict(gc_=gcl.short()), "d_g_cls_c8"),
        (split, dict(gx_=gbx.short()), "d_g_bbox_c8"), (split, dict(o_=loss.short()), "d_loss"),
    ]
    for fn, kw, name in refused:
        assert fn(**kw) == MPN_EINVAL and "footprint" in _err() and (name + " holds") in _err(), (fn.__name__, kw, _err())
    bad_args = [
        (wgrad, dict(H_=0)), (bias, dict(Cout_=0)), (pool, dict(C2=0)), (dpack, dict(Cin_=0)), (wpack, dict(Cin_=0)),
        (roi, dict(n1=N + 1)), (roi, dict(n0=3, n1=2)), (roi, dict(n0=-1)), (roi, dict(layout=2)), (roi, dict(layout=1, B_=2)), (roi, dict(layout=1, Mp_=N - 1)),
        (roi, dict(rule=2)), (roi, dict(PH_=0)),
        (split, dict(B_=0)), (split, dict(Mp_=B - 1)), (split, dict(k=Kc)), (split, dict(k=-1)),
    ]
    for fn, kw in bad_args:
        assert fn(**kw) == MPN_EINVAL and "invalid argument" in _err(), (fn.__name__, kw, _err())
    for buf in (xm, gm, part, dw, db, px, py, pd, w, tmp, wpk_t, zb, wino_t, wino, rg0, rg1, ram, rro, ro0, ro1, cls, box, rois, gt, gcl, gbx, loss):
        assert _is_sent(buf.read()), "a refused call wrote something"
