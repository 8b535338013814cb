"""The layout converters, weight packers, image transforms, the halo re-layer, the plain 2x2 pools and the shard and record packers, one
launch at a time and BIT FOR BIT against tests/layout_np.py (checked on the CPU in tests/test_layout_ref_cpu.py).  All of them are data
movement or arithmetic with one stated rounding, so no comparison here has a tolerance.  Until now they ran only inside whole layers and
pipelines: fresh zero-filled allocations, shapes that are multiples of 8, tolerances of 1e-4 — where an unwritten pad lane, a record written
into a halo or a row read past M cannot show.

The kernels are reached through the mpn_debug_* pass-throughs of layout_debug.hip and, for kernels local to a translation unit, of
pipeline.hip, graph_pool.hip and resnet.hip (debug flavour only; rules in layout_debug.h): raw device pointers, the product's own launcher
or the call site's grid, a byte count per buffer that turns a layout mistake of this file into MPN_EINVAL, and a refusal of pointers off the
alignment of the kernel's vector accesses.  maxpool2x2_nchw_kernel and pack_det_record_kernel have public entries and are called through them.

Common setup (Buf, twice, _is_sent, _same, _bits_acc are the training kernel modules').  Every device buffer sits between two guard zones of
256 floats holding the sentinel NaN 0x7FA5A5A5, which must survive every launch.  What the contract says is NOT WRITTEN holds the sentinel
before the launch and must keep its bits: the expected image of an output is the restatement laid over a sentinel fill, compared whole.  What
it says is NOT READ holds NaN (the ordinary values hold none, so one that is read shows in the output).  Inputs are read back unchanged.
Every case runs twice on fresh buffers and gives the same bits.  Values: magnitudes in [2^-6, 2^3], exact zeros, -0.0, +-inf, a denormal,
FLT_MAX.

Contracts as tested, per kernel (DESIGN.md section 13.17 has the table): nchw_to_c8p writes the H x W interior of every block, pad channels
+0.0, never halo or pitch padding; c8p_to_nchw never reads those.  rowmajor_to_c8 writes rows < M of chunks < ceil(K / 8), pad lanes +0.0,
and NOTHING else: a GEMM whose packed weight is rounded to K64 reads chunks up to K64 / 8 and rows up to Mp that this converter does not
write — their owner is the caller: mpn_linear_forward clears the whole K64 operand (hipMemsetAsync) before it converts, the one product call
site there is, and the debug GEMM entry does the same.  c8p_zero_halos writes +0.0 into exactly the non-interior records of each listed
map, both halves, whatever the number of launches (kHaloMax = 24 maps each).  The 2x2 pools never read the halo (2^100 and NaN there) and
follow `v > m from -inf`.  The shard kernels: rows at and beyond n_local of a row record +0.0, rows at and beyond the clamped count of a class
record / table untouched, keep_idx ints carried through the float-typed record bit for bit.

What the module found.  No kernel failed its contract.  Looked for and not found: an unwritten pad lane or pad row that the contract says is
written; a store into a halo, pitch padding, separator or spare mosaic cell; a read of a row, lane, halo or pad channel the contract says is
not read; an index that wraps or a guard off by one at C % 8 != 0, Cout % 128 != 0, H or W of 1, M = 1; a missed or doubled halo record at
the boundary between two launches or two descriptors; a division by base = 0 in shard_owner at N < world; a run-to-run difference.  One
hole was found beside them and is fixed: image_transform_c8p / image_transform_canvas_c8p / rn_image_transform take `swap` unchecked (a plane
index outside 0..2 reads outside the image) and mpn_frcnn_create* passed mpn_frcnn_config.tf_swap to them as given, where mpn_image_transform
has always refused such a value.  check_config now refuses it before a handle exists (test_create_refuses_swap_outside_planes), dense.h says
whose check it is, and the debug entries refuse it themselves.
Equivalent mutants (two behaviours, the same bits — a check cannot tell them apart): f2bf on a denormal input, flushed or
rounded, wherever the input is below 2^-134 (the values' 1e-42 and the image's 2^-140 both give bf16 0 either way; the one weight of 2^-130
does tell them apart: the device keeps it).  A third one is in the mutation table below.

MEASURED on the MI355X: 240 tests, 1127 whole-buffer comparisons over 9.6 million 32-bit words (the ACC lines), none differing; two runs in a
row print identical ACC lines; the module's wall time is 2.7 s.  Per kernel: shard_pack_classes 234, shard_unpack_classes 216, the C8P and
C8I image transforms 128 each (bf16: 32), pack_conv_generic 72, pack_conv_w 64, maxpool2x2_c8p 30, the four trunk converters 20 each,
pack_conv_bf16 18, c8p_zero_halos 18, maxpool2x2_nchw 15, pack_conv_w_first 12, shard_pack_rows 10, pack_det_record 10, shard_unpack_rows 8,
the three C8I converters 8 each, permute_w3 6, im2col3_c8i 6, unpack_pooled 5, copy_cols 5, the mosaic pair 3 each.

Mutations tried on scratch copies of the debug library (MI355X; each only changes what memory inside the tests' allocations is written or
read — the `<=` guards reach at most 84 floats into the 256-float guard zone behind a table), with the first test that fails on each and
how many do; all 31 are caught:
  nchw_to_c8p_kernel's store row y + 1 as y (halo offset dropped)              test_nchw_to_c8p[1-1-1] (all 20)
  c8p_to_nchw_kernel's lane c & 7 as c % 4                                     test_c8p_to_nchw[8-1-1] (the 12 with C >= 8)
  rowmajor_to_c8_kernel's k < K as k <= K                                      test_rowmajor_to_c8[1-1] (the 16 with K % 8 != 0)
  c8_to_rowmajor_kernel's pitch Mp as M                                        test_c8_to_rowmajor[1-9] (the 6 with N > 8 and M != Mp)
  pack_conv_w_kernel's ci < Cin as ci <= Cin                                   test_pack_conv_weights[3-1-0] (the 16 with Cin % 8 != 0)
  pack_conv_w_first_kernel's cin = 2 p + half as 2 half + p                    test_pack_conv_weights_first[3-1] (the 8 with Cin > 1)
  image_transform_c8p_kernel's second half-record not stored                   test_image_transform_c8p (all 4)
  image_transform_canvas_c8p_kernel's y < H && x < W as y < H                  test_image_transform_c8p (all 4)
  c8p_zero_halos_kernel's row = d.H + ri as d.H + ri - 1                       test_c8p_zero_halos[1] (all 5) and the every-geometry test
  c8p_zero_halos_kernel's descriptor search g >= first[k + 1] as g >          test_c8p_zero_halos[24], [25], [49]
  c8p_zero_halos_kernel's second half-record skipped                           test_c8p_zero_halos[1] (all 5) and the every-geometry test
  maxpool2x2_c8p_kernel's yy < H && xx < W as <= (reads the halo)              test_maxpool2x2_c8p[3-1-1] (the 9 with an odd H or W)
  maxpool2x2_nchw_kernel's v > m as v >= m                                     test_maxpool2x2_nchw[3-2-2] (the 12 with a -0.0 / +0.0 window)
  unpack_pooled_kernel's lane c & 7 as c % 4                                   test_unpack_pooled[1-9-4-3] (the 4 with C >= 8)
  copy_cols_kernel without col0                                                test_copy_cols[1-5-2-3] (the 3 with col0 > 0)
  shard_pack_rows_kernel's pass pitch n_local as chunk                         test_shard_rows[7-3-2-21] (the one case with P > 1)
  shard_unpack_rows_kernel's box plane offset dropped                          test_shard_rows (all 4)
  shard_pack_classes_kernel's i >= n as i > n (one row more)                   test_shard_classes[1-1] (all 12)
  shard_unpack_classes_kernel's i >= n as i > n                                test_shard_classes[1-1] (10 of 12)
  pack_det_record_kernel's t / 6 < n as <=                                     test_pack_det_record[1], [100]
  c8i_to_c8p_kernel's plane pitch as H * W                                     test_c8i_c8p_pixel_major[3-1-1] (the 3 with Cb = 3 and H * W below the pitch)
  c8p_to_c8i_kernel's column x + 1 as x                                        test_c8i_c8p_pixel_major (all 8)
  c8i_to_pixel_major_kernel's two halves swapped                               test_c8i_c8p_pixel_major (all 8)
  image_transform_c8i_kernel's planes 1 and 2 swapped                          test_image_transform_c8i (all 4)
  image_transform_c8i_bf16_kernel's last zero store dropped                    test_image_transform_c8i (all 4)
  c8i_to_mosaic_kernel's cell height H + 1 as H                                test_mosaic[5-7-7-2], [6-3-4-3] (the two with a second mosaic row)
  mosaic_to_c8i_kernel's cell width W + 1 as W                                 test_mosaic[5-7-7-2], [6-3-4-3] (the two with a second mosaic column)
  im2col3_c8i_kernel without its ky < KH check                                 test_im2col3_c8i (all 6)
  permute_w3_kernel's channel c as (c + 1) % 3                                 test_permute_w3 (all 6)
  pack_conv_generic_kernel's ci < Cin as ci <= Cin                             test_pack_conv_graph (the 12 with Cin % 8 != 0)
  pack_conv_bf16_kernel's ci < Cin as ci <= Cin                                test_pack_conv_graph (all 18: Cin = 8 has a second, zero chunk)
The descriptor-search mutant is equivalent wherever map k + 1 starts where map k ends: the record it misroutes lands on the next map's own
first halo record, which is zeroed either way.  test_c8p_zero_halos[2] and the twelve adjacent allocations therefore pass on it; the lists
of 24 and more, whose maps lie 256 sentinel floats apart, lose four floats of a gap to it.
"""
import ctypes as C
import functools
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layout_np as L  # noqa: E402
import test_gpu_train_conv_kernels_numerics as TCK  # noqa: E402  (_bits_acc, _is_sent, _sent_i)
import test_gpu_train_kernels_numerics as T  # noqa: E402  (Buf, twice, _sent, _same: one setup for all the kernel modules)

pytestmark = pytest.mark.gpu

F32 = np.float32
SENT, SENT_F = L.SENT, L.SENT_F
MPN_EINVAL = -1
GUARD = T.GUARD
Buf, twice = T.Buf, T.twice
_sent, _same = T._sent, T._same
_bits_acc, _is_sent, _sent_i = TCK._bits_acc, TCK._is_sent, TCK._sent_i
ci, cs, vp, cd = C.c_int, C.c_size_t, C.c_void_p, C.c_double
I3, D3 = ci * 3, cd * 3
BIG = F32(2.0 ** 100)


@functools.lru_cache(maxsize=None)
def _dbg():
    lib = T._dbg()
    b = [vp, cs]  # a buffer and its size in bytes
    lib.mpn_debug_nchw_to_c8p.argtypes = b + [ci, ci, ci] + b
    lib.mpn_debug_c8p_to_nchw.argtypes = b + [ci, ci, ci] + b
    lib.mpn_debug_rowmajor_to_c8.argtypes = b + [ci, ci] + b
    lib.mpn_debug_c8_to_rowmajor.argtypes = b + [ci, ci] + b
    lib.mpn_debug_unpack_pooled.argtypes = b + [ci, ci, ci, ci] + b
    lib.mpn_debug_copy_cols.argtypes = b + [ci, ci, ci, ci] + b
    lib.mpn_debug_pack_conv_weights.argtypes = b + b + [ci, ci] + b + b
    lib.mpn_debug_pack_conv_weights_first.argtypes = b + [ci, ci] + b
    lib.mpn_debug_image_transform_c8p.argtypes = b + [ci, ci, C.POINTER(I3), cd, C.POINTER(D3), C.POINTER(D3), ci, ci, ci, ci] + b
    lib.mpn_debug_c8p_zero_halos.argtypes = [ci, vp, vp, vp, vp, vp]
    lib.mpn_debug_maxpool2x2_c8p.argtypes = b + [ci, ci, ci] + b
    lib.mpn_maxpool2x2_ceil_forward.argtypes = [vp, ci, ci, ci, vp, vp]
    lib.mpn_pack_det_record.argtypes = [vp, vp, ci, vp, vp]
    lib.mpn_debug_shard_pack_rows.argtypes = b + b + [ci] * 5 + b
    lib.mpn_debug_shard_unpack_rows.argtypes = b + [ci] * 4 + b + b
    lib.mpn_debug_shard_pack_classes.argtypes = b + b + b + b + [ci] * 4 + b
    lib.mpn_debug_shard_unpack_classes.argtypes = b + [ci] * 3 + b + b + b + b
    lib.mpn_debug_c8i_c8p.argtypes = b + b + [ci] * 4
    lib.mpn_debug_c8i_to_pixel_major.argtypes = b + [ci] * 3 + b
    lib.mpn_debug_c8i_mosaic.argtypes = b + b + [ci] * 7
    lib.mpn_debug_im2col3_c8i.argtypes = b + [ci] * 6 + b
    lib.mpn_debug_permute_w3.argtypes = b + [ci, ci] + b
    lib.mpn_debug_pack_conv_graph.argtypes = b + b + [ci] * 4 + b + b
    lib.mpn_debug_image_transform_c8i.argtypes = b + [ci, ci, C.POINTER(I3), cd, C.POINTER(D3), C.POINTER(D3), ci, ci] + b + b
    return lib


def _err():
    return _dbg().mpn_last_error().decode()


def _ok(rc):
    assert rc == 0, (rc, _err())


def _invalid(rc):
    assert rc == MPN_EINVAL and "invalid argument" in _err(), (rc, _err())


def _short(rc, name):
    assert rc == MPN_EINVAL and "footprint" in _err() and (name + " holds") in _err(), (rc, name, _err())


def _misaligned(rc, name):
    assert rc == MPN_EINVAL and (name + " must be") in _err() and "aligned" in _err(), (rc, name, _err())


def B(buf, short=0, off=0):
    """(pointer, bytes) as the entries take a buffer; `short` bytes fewer, `off` bytes further"""
    return (vp(buf.ptr + off), 4 * buf.n - short)


NULLB = (None, 0)


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _exact(tag, got, want):
    """whole-buffer bit comparison (written AND unwritten parts) with its ACC line"""
    got, want = _words(got), _words(want)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = int((got != want).sum())
    print("ACC %-72s words differ in %d of %d" % (tag, bad, got.size))
    assert bad == 0, tag


# ---- nchw_to_c8p / c8p_to_nchw --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", L.MAP_HW)
@pytest.mark.parametrize("C_", L.MAP_C)
def test_nchw_to_c8p(dev, C_, H, W):
    x = L.values([C_, H, W, 1], (C_, H, W))
    want = L.c8p_pack(x, pad=0.0, halo=SENT_F, pitch=SENT_F)   # interior of every block written (pad channels +0.0), nothing else

    def call():
        xb, ob = Buf(x), Buf(_sent(*want.shape))
        _ok(_dbg().mpn_debug_nchw_to_c8p(*B(xb), C_, H, W, *B(ob)))
        out = ob.read()
        assert _same(xb.read(), x), "the input was written"
        return (out,)
    _exact("nchw_to_c8p C=%d %dx%d" % (C_, H, W), twice(call)[0], want)


@pytest.mark.parametrize("H,W", L.MAP_HW)
@pytest.mark.parametrize("C_", L.MAP_C)
def test_c8p_to_nchw(dev, C_, H, W):
    x = L.values([C_, H, W, 2], (C_, H, W))
    m = L.c8p_pack(x, pad=SENT_F, halo=SENT_F, pitch=SENT_F)   # halo, pitch padding, pad channels: NaN, never read

    def call():
        mb, ob = Buf(m), Buf(_sent(C_, H, W))
        _ok(_dbg().mpn_debug_c8p_to_nchw(*B(mb), C_, H, W, *B(ob)))
        out = ob.read()
        assert _same(mb.read(), m), "the input was written"
        return (out,)
    _exact("c8p_to_nchw C=%d %dx%d" % (C_, H, W), twice(call)[0], x)


# ---- rowmajor_to_c8 / c8_to_rowmajor / unpack_pooled / copy_cols ----------------------------------------------------------------------------
@pytest.mark.parametrize("K", L.ROWMAJOR_K)
@pytest.mark.parametrize("M", L.ROWMAJOR_M)
def test_rowmajor_to_c8(dev, M, K):
    """Rows m >= M up to Mp keep the sentinel, pad lanes of the last chunk are +0.0, and the chunk after ceil(K / 8) - 1 (one more than the
    footprint, the K64 operand's next one) is not written: the K64 chunks and the pad rows a GEMM reads are the CALLER's to zero
    (mpn_linear_forward: hipMemsetAsync of the whole operand before the conversion)."""
    x = L.values([M, K, 3], (M, K))
    Mp, q = L.lin_mp(M), L.cdiv(K, 8)
    want = _sent(q + 1, Mp, 8)
    want[:q] = L.c8_pack(x, Mp, lane_fill=0.0, row_fill=SENT_F)

    def call():
        xb, ob = Buf(x), Buf(_sent(q + 1, Mp, 8))
        _ok(_dbg().mpn_debug_rowmajor_to_c8(*B(xb), M, K, *B(ob)))
        out = ob.read()
        assert _same(xb.read(), x)
        return (out,)
    _exact("rowmajor_to_c8 M=%d K=%d" % (M, K), twice(call)[0], want)


@pytest.mark.parametrize("N", L.ROWMAJOR_K)
@pytest.mark.parametrize("M", L.ROWMAJOR_M)
def test_c8_to_rowmajor(dev, M, N):
    x = L.values([M, N, 4], (M, N))
    m = L.c8_pack(x, L.lin_mp(M), lane_fill=SENT_F, row_fill=SENT_F)   # rows >= M, lanes >= N: never read

    def call():
        mb, ob = Buf(m), Buf(_sent(M, N))
        _ok(_dbg().mpn_debug_c8_to_rowmajor(*B(mb), M, N, *B(ob)))
        out = ob.read()
        assert _same(mb.read(), m)
        return (out,)
    _exact("c8_to_rowmajor M=%d N=%d" % (M, N), twice(call)[0], x)


POOLED_CASES = ((1, 1, 1, 1), (1, 9, 4, 3), (3, 9, 4, 5), (5, 17, 49, 128), (130, 8, 2, 256))  # (N, C, PP, Mp): M = 1, ragged C, Mp > N


@pytest.mark.parametrize("N,C_,PP,Mp", POOLED_CASES)
def test_unpack_pooled(dev, N, C_, PP, Mp):
    x = L.values([N, C_, PP, 5], (N, C_, PP))
    m = L.pooled_pack(x, Mp, fill=SENT_F)

    def call():
        mb, ob = Buf(m), Buf(_sent(N, C_ * PP))
        _ok(_dbg().mpn_debug_unpack_pooled(*B(mb), N, C_, PP, Mp, *B(ob)))
        out = ob.read()
        assert _same(mb.read(), m)
        return (out,)
    _exact("unpack_pooled N=%d C=%d PP=%d Mp=%d" % (N, C_, PP, Mp), twice(call)[0], x.reshape(N, C_ * PP))


COLS_CASES = ((1, 5, 2, 3), (1, 9, 2, 4), (3, 9, 0, 4), (257, 21, 7, 13), (64, 4, 0, 4))  # (M, ld, col0, ncols)


@pytest.mark.parametrize("M,ld,col0,ncols", COLS_CASES)
def test_copy_cols(dev, M, ld, col0, ncols):
    x = L.values([M, ld, col0, 6], (M, ncols))
    src = _sent(M, ld)
    src[:, col0:col0 + ncols] = x   # every other column: NaN, never read

    def call():
        sb, ob = Buf(src), Buf(_sent(M, ncols))
        _ok(_dbg().mpn_debug_copy_cols(*B(sb), ld, col0, M, ncols, *B(ob)))
        out = ob.read()
        assert _same(sb.read(), src)
        return (out,)
    _exact("copy_cols M=%d ld=%d col0=%d ncols=%d" % (M, ld, col0, ncols), twice(call)[0], x)


# ---- pack_conv_weights / pack_conv_weights_first ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", (0, 1))
@pytest.mark.parametrize("Cout", L.CONV_COUT)
@pytest.mark.parametrize("Cin", L.CONV_CIN)
def test_pack_conv_weights(dev, Cin, Cout, bias):
    w, b = L.values([Cin, Cout, 7], (Cout, Cin, 3, 3)), L.values([Cin, Cout, 8], (Cout,))
    want_w = L.conv_pack(w)                                   # every element of [nch][9][CoutP][8] written, pad +0.0
    want_b = np.zeros(L.conv_coutp(Cout), F32)
    if bias:
        want_b[:Cout] = b

    def call():
        wb, bb, ob, obb = Buf(w), Buf(b), Buf(_sent(*want_w.shape)), Buf(_sent(want_b.size))
        _ok(_dbg().mpn_debug_pack_conv_weights(*B(wb), *(B(bb) if bias else NULLB), Cin, Cout, *B(ob), *B(obb)))
        out = ob.read(), obb.read()
        assert _same(wb.read(), w) and _same(bb.read(), b)
        return out
    got_w, got_b = twice(call)
    _exact("pack_conv_w Cin=%d Cout=%d bias=%d" % (Cin, Cout, bias), got_w, want_w)
    _exact("pack_conv_w bias Cin=%d Cout=%d bias=%d" % (Cin, Cout, bias), got_b, want_b)


@pytest.mark.parametrize("Cout", L.CONV_COUT)
@pytest.mark.parametrize("Cin", L.FIRST_CIN)
def test_pack_conv_weights_first(dev, Cin, Cout):
    w = L.values([Cin, Cout, 9], (Cout, Cin, 3, 3))
    want = L.conv_first_pack(w)

    def call():
        wb, ob = Buf(w), Buf(_sent(*want.shape))
        _ok(_dbg().mpn_debug_pack_conv_weights_first(*B(wb), Cin, Cout, *B(ob)))
        out = ob.read()
        assert _same(wb.read(), w)
        return (out,)
    _exact("pack_conv_w_first Cin=%d Cout=%d" % (Cin, Cout), twice(call)[0], want)


# ---- the image transforms ----------------------------------------------------------------------------------------------------------------------
IMAGE_CFG = tuple(itertools.product(L.IMAGE_SWAPS, L.IMAGE_SCALES, (0, 1)))


@pytest.mark.parametrize("H,W", L.MAP_HW)
def test_image_transform_c8p(dev, H, W):
    """The plain form and the canvas form at (Hc, Wc) = (H, W), (H + 1, W), (H, W + 5): the whole canvas interior written (the image, +0.0 in
    channels 3..7 and outside the image), halo and pitch padding untouched.  Pixel (0, 0) of output channel 0 cancels to a denormal, pixels
    (0, 0) and (0, 1) of channel 1 are float rounding ties of the double result (tests/layout_np.py image_case)."""
    for swap, scale, has_std in IMAGE_CFG:
        img, mean = L.image_case(H, W, swap, scale, 1)
        t = L.image_transform(img, swap, scale, mean, L.IMAGE_STD, has_std)
        forms = [(0, H, W)] + [(1, H + a, W + b) for a, b in L.CANVAS_EXTRA]
        for canvas, Hc, Wc in forms:
            want = L.image_c8p(t, Hc, Wc, outside=SENT_F)

            def call():
                ib, ob = Buf(img), Buf(_sent(*want.shape))
                _ok(_dbg().mpn_debug_image_transform_c8p(*B(ib), H, W, I3(*swap), scale, D3(*mean), D3(*L.IMAGE_STD), has_std, canvas, Hc, Wc, *B(ob)))
                out = ob.read()
                assert _same(ib.read(), img)
                return (out,)
            _exact("image_transform_c8p %dx%d canvas=%d %dx%d swap=%s scale=%g std=%d" % (H, W, canvas, Hc, Wc, swap, scale, has_std), twice(call)[0], want)


@pytest.mark.parametrize("H,W", L.MAP_HW)
def test_image_transform_c8i(dev, H, W):
    """fp32: records [H * W][8] (channels 3..7 +0.0) and, when asked for, the [3][H][W] planes; rows beyond H * W untouched.  bf16: two planes
    [2][pitch][8] of 16-bit values, plane 1 and channels 3..7 zero, rows beyond H * W untouched; f2bf restated on integers (round to nearest even)."""
    pitch = L.c8i_pitch(H * W)
    for swap, scale, has_std in IMAGE_CFG:
        img, mean = L.image_case(H, W, swap, scale, 2)
        t = L.image_transform(img, swap, scale, mean, L.IMAGE_STD, has_std)
        rec = np.zeros((H * W, 8), F32)
        rec[:, :3] = t.reshape(3, -1).T
        want32 = _sent(pitch, 8)
        want32[:H * W] = rec
        want16 = np.full(pitch * 8, SENT, np.uint32).view(np.uint16).reshape(2, pitch, 8).copy()
        want16[:, :H * W] = 0
        want16[0, :H * W] = L.f2bf_bits(rec)
        tag = "%dx%d swap=%s scale=%g std=%d" % (H, W, swap, scale, has_std)
        for planar in (0, 1):
            def call():
                ib, ob, pb = Buf(img), Buf(_sent(pitch, 8)), Buf(_sent(3, H, W))
                _ok(_dbg().mpn_debug_image_transform_c8i(*B(ib), H, W, I3(*swap), scale, D3(*mean), D3(*L.IMAGE_STD), has_std, 0, *B(ob),
                                                         *(B(pb) if planar else NULLB)))
                out = ob.read(), pb.read()
                assert _same(ib.read(), img)
                return out
            got, gp = twice(call)
            _exact("image_transform_c8i " + tag + " planar=%d" % planar, got, want32)
            _exact("image_transform_c8i planes " + tag + " planar=%d" % planar, gp, t if planar else _sent(3, H, W))

        def call16():
            ib, ob = Buf(img), Buf(_sent(pitch * 8))   # 2 * pitch * 8 16-bit values
            _ok(_dbg().mpn_debug_image_transform_c8i(*B(ib), H, W, I3(*swap), scale, D3(*mean), D3(*L.IMAGE_STD), has_std, 1, *B(ob), *NULLB))
            out = ob.read()
            assert _same(ib.read(), img)
            return (out,)
        _exact("image_transform_c8i_bf16 " + tag, twice(call16)[0], want16.reshape(-1).view(np.uint32))


# ---- c8p_zero_halos ----------------------------------------------------------------------------------------------------------------------------
def _halo_run(geos, gaps):
    """maps of the (C, H, W) in `geos` in ONE allocation, map i + 1 starting gaps[i] floats after map i ends (0: adjacent allocations), all
    filled with the sentinel -> (the buffer after the call, the expected buffer)"""
    sizes = [L.cdiv(c, 8) * L.act_hp(h) * L.act_wp(w) * 8 for c, h, w in geos]
    offs, pos = [], 0
    for i, s in enumerate(sizes):
        offs.append(pos)
        pos += s + (gaps[i] if i < len(gaps) else 0)
    total = offs[-1] + sizes[-1]
    want = _sent(total)
    for (c, h, w), o, s in zip(geos, offs, sizes):
        v = want[o:o + s].reshape(L.cdiv(c, 8), L.act_hp(h), L.act_wp(w), 8)
        v[L.halo_mask(c, h, w)] = 0.0   # exactly the non-interior records, both halves; the interior keeps the sentinel
    n = len(geos)

    def call():
        buf = Buf(_sent(total))
        ptrs = (vp * n)(*[buf.ptr + 4 * o for o in offs])
        byts = (cs * n)(*[4 * s for s in sizes])
        cc, hh, ww = ((ci * n)(*[g[k] for g in geos]) for k in range(3))
        _ok(_dbg().mpn_debug_c8p_zero_halos(n, ptrs, byts, cc, hh, ww))
        return (buf.read(),)
    return twice(call)[0], want


@pytest.mark.parametrize("n", L.HALO_N)
def test_c8p_zero_halos(dev, n):
    """n = 1, 2: one launch; 24: one full table; 25: a second launch of one map; 49: three launches.  Mixed geometries in every list; maps 0
    and 1 are adjacent allocations (nothing between them), the others 256 sentinel floats apart (a guard between two maps)."""
    geos = L.halo_list(n)
    got, want = _halo_run(geos, [0] + [GUARD] * (n - 2))
    _exact("c8p_zero_halos n=%d" % n, got, want)


def test_c8p_zero_halos_every_geometry_alone_and_adjacent(dev):
    for c, hw in itertools.product(L.HALO_C, L.HALO_HW):
        got, want = _halo_run([(c,) + hw], [])
        _exact("c8p_zero_halos alone C=%d %dx%d" % ((c,) + hw), got, want)
    geos = [(c,) + hw for hw in L.HALO_HW for c in L.HALO_C]
    got, want = _halo_run(geos, [0] * (len(geos) - 1))       # twelve adjacent allocations
    _exact("c8p_zero_halos 12 adjacent", got, want)


def test_c8p_zero_halos_none(dev):
    _ok(_dbg().mpn_debug_c8p_zero_halos(0, None, None, None, None, None))   # n = 0 launches nothing


# ---- the 2x2 pools -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", L.POOL_HW)
@pytest.mark.parametrize("C_", L.POOL_C)
def test_maxpool2x2_c8p(dev, C_, H, W):
    """The input's halo and pitch padding hold 2^100 (finite and above every value: a `>` that reads the halo for the odd last row or column
    shows), then NaN.  The output's halo keeps the sentinel; its pad channels are the pool of the input's +0.0 pad channels."""
    x = L.pool_input(C_, H, W, 3)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    want = L.c8p_pack(L.maxpool2x2(x), pad=0.0, halo=SENT_F, pitch=SENT_F)
    for name, outside in (("2^100", BIG), ("NaN", SENT_F)):
        m = L.c8p_pack(x, pad=0.0, halo=outside, pitch=outside)

        def call():
            mb, ob = Buf(m), Buf(_sent(*want.shape))
            _ok(_dbg().mpn_debug_maxpool2x2_c8p(*B(mb), C_, H, W, *B(ob)))
            out = ob.read()
            assert _same(mb.read(), m)
            return (out,)
        _exact("maxpool2x2_c8p C=%d %dx%d halo %s" % (C_, H, W, name), twice(call)[0], want)
    assert want.shape[1:3] == (L.act_hp(Ho), L.act_wp(Wo))


@pytest.mark.parametrize("H,W", L.POOL_HW)
@pytest.mark.parametrize("C_", L.POOL_C)
def test_maxpool2x2_nchw(dev, C_, H, W):
    x = L.pool_input(C_, H, W, 4)
    want = L.maxpool2x2(x)

    def call():
        xb, ob = Buf(x), Buf(_sent(*want.shape))
        _ok(_dbg().mpn_maxpool2x2_ceil_forward(vp(xb.ptr), C_, H, W, vp(ob.ptr), None))
        out = ob.read()
        assert _same(xb.read(), x)
        return (out,)
    _exact("maxpool2x2_nchw BC=%d %dx%d" % (C_, H, W), twice(call)[0], want)


# ---- the shard records ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,world,P,C_", L.SHARD_ROWS)
def test_shard_rows(dev, N, world, P, C_):
    """Every rank packs its tables; the records, concatenated, unpack to the unsharded tables.  (3, 4, 1, 2): N < world — rank 3 owns nothing
    (null tables, a record of +0.0) and shard_owner's base is 0."""
    sc, bb = L.values([N, world, P, C_, 1], (P, N, C_)), L.values([N, world, P, C_, 2], (P, N, 4 * C_))
    rec_floats = P * L.cdiv(N, world) * 5 * C_
    recs = []
    for rank in range(world):
        lo, hi = L.shard_bounds(N, world, rank)
        s_loc, b_loc = np.ascontiguousarray(sc[:, lo:hi]), np.ascontiguousarray(bb[:, lo:hi])
        want = L.shard_rows_record(s_loc, b_loc, N, world, rank, P, C_)

        def call():
            ob = Buf(_sent(rec_floats))
            if hi > lo:
                sb, bbuf = Buf(s_loc), Buf(b_loc)
                _ok(_dbg().mpn_debug_shard_pack_rows(*B(sb), *B(bbuf), N, world, rank, P, C_, *B(ob)))
                assert _same(sb.read(), s_loc) and _same(bbuf.read(), b_loc)
            else:
                _ok(_dbg().mpn_debug_shard_pack_rows(*NULLB, *NULLB, N, world, rank, P, C_, *B(ob)))
            return (ob.read(),)
        got = twice(call)[0]
        _exact("shard_pack_rows N=%d world=%d rank=%d P=%d C=%d" % (N, world, rank, P, C_), got, want)
        recs.append(got)
    allr = np.stack(recs)

    def call2():
        ab, sb, bbuf = Buf(allr), Buf(_sent(P, N, C_)), Buf(_sent(P, N, 4 * C_))
        _ok(_dbg().mpn_debug_shard_unpack_rows(*B(ab), N, world, P, C_, *B(sb), *B(bbuf)))
        out = sb.read(), bbuf.read()
        assert _same(ab.read(), allr)
        return out
    s2, b2 = twice(call2)
    _exact("shard_unpack_rows scores N=%d world=%d P=%d C=%d" % (N, world, P, C_), s2, sc)
    _exact("shard_unpack_rows boxes N=%d world=%d P=%d C=%d" % (N, world, P, C_), b2, bb)
    js, jb = L.shard_rows_join(allr, N, world, P, C_)
    assert _same(js, sc) and _same(jb, bb)


def _class_case(n_cls, rows, seed):
    rng = np.random.default_rng([n_cls, rows, seed])
    keep, voted = L.values([n_cls, rows, seed, 1], (n_cls, rows, 5)), L.values([n_cls, rows, seed, 2], (n_cls, rows, 5))
    kidx = rng.integers(0, 2 ** 20, (n_cls, rows)).astype(np.int32)
    flat = kidx.reshape(-1)   # every third index: a bit pattern that is a NaN as a float (quiet, signalling, all ones, one off the sentinel)
    sp = np.array([0x7FC00001, 0x7F800001, 0xFFFFFFFF, 0x7FA5A5A4], np.uint32).view(np.int32)
    flat[::3] = sp[np.arange(flat[::3].size) % 4]
    n_keep = rng.integers(0, rows + 1, n_cls).astype(np.int32)
    special = [0, rows, -3, rows + 7]                      # 0, rows, a negative count and one above rows: both clamped
    n_keep[:len(special)] = special[:n_cls]
    if n_cls == 1:
        n_keep[0] = rows + 7
    return keep, kidx, n_keep, voted


@pytest.mark.parametrize("world", L.SHARD_WORLD)
@pytest.mark.parametrize("n_cls", L.SHARD_CLS)
def test_shard_classes(dev, n_cls, world):
    """Pack every rank's class record, compare it whole (rows at and beyond each clamped count keep the sentinel, slots past the rank's range
    hold count 0), concatenate, unpack, compare the tables whole (rows at and beyond the count keep the sentinel).  keep_idx values whose bit
    pattern is a NaN as a float cross the float-typed record bit for bit."""
    for rows, voting in itertools.product(L.SHARD_NROWS, (0, 1)):
        keep, kidx, n_keep, voted = _class_case(n_cls, rows, world)
        if n_cls == 1 and rows > 1:
            n_keep[0] = (0, rows, -3, rows + 7)[(world + voting) % 4]
        v = voted if voting else None
        recs = []
        for rank in range(world):
            want = L.shard_class_record(keep, kidx, n_keep, v, n_cls, world, rank, rows)

            def call():
                kb, ib, nb, vb, ob = Buf(keep), Buf(kidx), Buf(n_keep), Buf(voted), Buf(_sent(want.size))
                _ok(_dbg().mpn_debug_shard_pack_classes(*B(kb), *B(ib), *B(nb), *(B(vb) if voting else NULLB), n_cls, world, rank, rows, *B(ob)))
                out = ob.read()
                assert _same(kb.read(), keep) and np.array_equal(ib.read(), kidx) and np.array_equal(nb.read(), n_keep) and _same(vb.read(), voted)
                return (out,)
            got = twice(call)[0]
            _exact("shard_pack_classes n_cls=%d world=%d rank=%d rows=%d voting=%d" % (n_cls, world, rank, rows, voting), got, want)
            recs.append(_words(got))
        allr = np.stack(recs)
        wk, wi, wn, wv = L.shard_class_join(allr, n_cls, world, rows, voting)

        def call2():
            ab, kb, ib, nb, vb = Buf(allr.view(F32)), Buf(_sent(n_cls, rows, 5)), Buf(_sent_i(n_cls, rows)), Buf(_sent_i(n_cls)), Buf(_sent(n_cls, rows, 5))
            _ok(_dbg().mpn_debug_shard_unpack_classes(*B(ab), n_cls, world, rows, *B(kb), *B(ib), *B(nb), *(B(vb) if voting else NULLB)))
            out = kb.read(), ib.read(), nb.read(), vb.read()
            assert np.array_equal(_words(ab.read()), allr)
            return out
        gk, gi, gn, gv = twice(call2)
        tag = "n_cls=%d world=%d rows=%d voting=%d" % (n_cls, world, rows, voting)
        _exact("shard_unpack_classes keep " + tag, gk, wk)
        _exact("shard_unpack_classes kidx " + tag, gi, wi)
        _exact("shard_unpack_classes voted " + tag, gv, wv if voting else _sent(n_cls, rows, 5))
        assert np.array_equal(gn, wn) and np.array_equal(gn, np.clip(n_keep, 0, rows))
        for c in range(n_cls):   # the joined tables are the unsharded ones up to each count
            n = gn[c]
            assert _same(gk[c, :n], keep[c, :n]) and np.array_equal(gi[c, :n], kidx[c, :n])


@pytest.mark.parametrize("top_cap", L.DET_CAP)
def test_pack_det_record(dev, top_cap):
    dets = L.values([top_cap, 10], (top_cap, 6))
    for n in (-3, 0, 1, top_cap, top_cap + 5):
        c = L.clamp_count(n, top_cap)
        src = dets.copy()
        src[c:] = SENT_F                                      # rows at and beyond the count: never read
        want = L.det_record(dets, n, top_cap)
        cnt = np.array([n], np.int32)

        def call():
            db, nb, ob = Buf(src), Buf(cnt), Buf(_sent(top_cap * 6 + 1))
            _ok(_dbg().mpn_pack_det_record(vp(db.ptr), vp(nb.ptr), top_cap, vp(ob.ptr), None))
            out = ob.read()
            assert _same(db.read(), src) and np.array_equal(nb.read(), cnt)
            return (out,)
        _exact("pack_det_record top_cap=%d n=%d" % (top_cap, n), twice(call)[0], want)


# ---- the graph executor's side -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", L.MAP_HW)
@pytest.mark.parametrize("Cb", L.C8I_CB)
def test_c8i_c8p_pixel_major(dev, Cb, H, W):
    """C8I pitch padding (rows H * W .. pitch) holds NaN on the way in and keeps the sentinel on the way out; the same for the C8P halo."""
    C_ = Cb * 8
    x = L.values([Cb, H, W, 11], (1, C_, H, W))
    c8i_in, c8p_in = L.c8i_pack(x, row_fill=SENT_F), L.c8p_pack(x[0], halo=SENT_F, pitch=SENT_F)
    c8i_want, c8p_want = c8i_in, c8p_in   # (the sentinel IS the NaN: what must not be read on one side must not be written on the other)
    tag = "Cb=%d %dx%d" % (Cb, H, W)

    def to_c8p():
        ib, ob = Buf(c8i_in), Buf(_sent(*c8p_want.shape))
        _ok(_dbg().mpn_debug_c8i_c8p(*B(ib), *B(ob), C_, H, W, 1))
        out = ob.read()
        assert _same(ib.read(), c8i_in)
        return (out,)
    _exact("c8i_to_c8p " + tag, twice(to_c8p)[0], c8p_want)

    def to_c8i():
        ob, ib = Buf(_sent(*c8i_want.shape)), Buf(c8p_in)
        _ok(_dbg().mpn_debug_c8i_c8p(*B(ob), *B(ib), C_, H, W, 0))
        out = ob.read()
        assert _same(ib.read(), c8p_in)
        return (out,)
    _exact("c8p_to_c8i " + tag, twice(to_c8i)[0], c8i_want)

    def to_pm():
        ib, ob = Buf(c8i_in), Buf(_sent(H * W, C_))
        _ok(_dbg().mpn_debug_c8i_to_pixel_major(*B(ib), C_, H, W, *B(ob)))
        out = ob.read()
        assert _same(ib.read(), c8i_in)
        return (out,)
    _exact("c8i_to_pixel_major " + tag, twice(to_pm)[0], L.pixel_major(x[0]))


@pytest.mark.parametrize("N,H,W,mx", L.MOSAIC)
def test_mosaic(dev, N, H, W, mx):
    """A mosaic laid out for N + 3 maps: separator rows and columns, the cells of maps >= N and the halo keep the sentinel on the way in and
    hold NaN, never read, on the way back; the round trip is the identity."""
    C_, cap = 16, N + L.MOSAIC_SPARE
    x = L.values([N, H, W, mx, 12], (N, C_, H, W))
    c8i, mos = L.c8i_pack(x, row_fill=SENT_F), L.mosaic_pack(x, cap, mx, fill=SENT_F)
    tag = "N=%d %dx%d mx=%d" % (N, H, W, mx)

    def fwd():
        ib, ob = Buf(c8i), Buf(_sent(*mos.shape))
        _ok(_dbg().mpn_debug_c8i_mosaic(*B(ib), *B(ob), C_, N, cap, H, W, mx, 1))
        out = ob.read()
        assert _same(ib.read(), c8i)
        return (out,)
    got = twice(fwd)[0]
    _exact("c8i_to_mosaic " + tag, got, mos)

    def back():
        ob, ib = Buf(_sent(*c8i.shape)), Buf(got)
        _ok(_dbg().mpn_debug_c8i_mosaic(*B(ob), *B(ib), C_, N, cap, H, W, mx, 0))
        out = ob.read()
        assert _same(ib.read(), got)
        return (out,)
    _exact("mosaic_to_c8i(c8i_to_mosaic(x)) " + tag, twice(back)[0], c8i)


@pytest.mark.parametrize("H,W", L.IM2COL_HW)
@pytest.mark.parametrize("KH,KW,stride,pad", L.IM2COL_K)
def test_im2col3_c8i(dev, KH, KW, stride, pad, H, W):
    img = L.values([KH, stride, H, W, 13], (3, H, W))
    want = L.im2col3(img, KH, KW, stride, pad, row_fill=SENT_F)   # k beyond KH * KW * 3 and outside taps +0.0; rows beyond OH * OW untouched

    def call():
        ib, ob = Buf(img), Buf(_sent(*want.shape))
        _ok(_dbg().mpn_debug_im2col3_c8i(*B(ib), H, W, KH, KW, stride, pad, *B(ob)))
        out = ob.read()
        assert _same(ib.read(), img)
        return (out,)
    _exact("im2col3_c8i %dx%d/%d pad %d on %dx%d" % (KH, KW, stride, pad, H, W), twice(call)[0], want)


@pytest.mark.parametrize("Cout,KK", tuple(itertools.product(L.PERMUTE_COUT, L.PERMUTE_KK)))
def test_permute_w3(dev, Cout, KK):
    w = L.values([Cout, KK, 14], (Cout, 3, KK))

    def call():
        wb, ob = Buf(w), Buf(_sent(Cout, KK * 3))
        _ok(_dbg().mpn_debug_permute_w3(*B(wb), Cout, KK, *B(ob)))
        out = ob.read()
        assert _same(wb.read(), w)
        return (out,)
    _exact("permute_w3 Cout=%d KK=%d" % (Cout, KK), twice(call)[0], L.permute_w3(w))


@pytest.mark.parametrize("KK,Cin,Cout", tuple(itertools.product(L.GCONV_KK, L.GCONV_CIN, L.GCONV_COUT)))
def test_pack_conv_graph(dev, KK, Cin, Cout):
    """pack_conv_generic_kernel (with and without a bias) and pack_conv_bf16_kernel (nch2: the chunk count rounded up to even, the added
    chunk zero; the bf16 bits compared as integers).  One weight is 2^-130, a float denormal that is NOT below bf16's smallest: round to
    nearest even keeps it (0x0008) where a flush would give 0."""
    w, b = L.values([KK, Cin, Cout, 15], (Cout, Cin, KK)), L.values([KK, Cin, Cout, 16], (Cout,))
    w[0, 0, 0] = F32(2.0 ** -130)
    CoutP = L.round_up(Cout, 128)
    want = L.gconv_pack(w)
    tag = "KK=%d Cin=%d Cout=%d" % (KK, Cin, Cout)
    for bias in (0, 1):
        want_b = np.zeros(CoutP, F32)
        if bias:
            want_b[:Cout] = b

        def call():
            wb, bb, ob, obb = Buf(w), Buf(b), Buf(_sent(*want.shape)), Buf(_sent(CoutP))
            _ok(_dbg().mpn_debug_pack_conv_graph(*B(wb), *(B(bb) if bias else NULLB), Cin, Cout, KK, 0, *B(ob), *B(obb)))
            out = ob.read(), obb.read()
            assert _same(wb.read(), w) and _same(bb.read(), b)
            return out
        gw, gb = twice(call)
        _exact("pack_conv_generic %s bias=%d" % (tag, bias), gw, want)
        _exact("pack_conv_generic bias %s bias=%d" % (tag, bias), gb, want_b)
    nch2 = L.round_up(L.cdiv(Cin, 8), 2)
    want16 = L.f2bf_bits(L.gconv_pack(w, nch=nch2))

    def call16():
        wb, ob = Buf(w), Buf(_sent(want16.size // 2))
        _ok(_dbg().mpn_debug_pack_conv_graph(*B(wb), *NULLB, Cin, Cout, KK, 1, *B(ob), *NULLB))
        out = ob.read()
        assert _same(wb.read(), w)
        return (out,)
    got16 = _words(twice(call16)[0]).view(np.uint16)
    bad = int((got16 != want16.reshape(-1)).sum())
    print("ACC %-72s bf16 values differ in %d of %d" % ("pack_conv_bf16 " + tag, bad, got16.size))
    assert bad == 0
    assert want16[0, 0, 0, 0] == 0x0008


def test_create_refuses_swap_outside_planes(dev):
    """Regression: a handle whose transformer names a plane outside 0..2 is refused at creation (it used to be created, and its first image
    was read out of bounds by the transform kernel)."""
    from multipathnet_amd import _lib, models
    cfg = [8, 8, "P", 16, "P", 16]   # tests/test_gpu_handle_lifetime.py's plain handle
    P = models.synthetic_params(cfg, pooled=7, fc_dim=32, n_classes=4, seed=1)
    for swap in ((2, 1, 3), (-1, 1, 0)):
        with pytest.raises(_lib.MpnError, match="tf_swap"):
            models.FastRCNN(P, cfg=cfg, pooled=7, spatial_scale=0.25, max_h=150, max_w=256, max_rois=64,
                            transformer=dict(mean=(1.0, 2.0, 3.0), std=None, scale=1.0, swap=swap))


# ---- refusals: every one returns before any launch (the buffers keep the sentinel) ------------------------------------------------------------
def test_refusals(dev):
    d = _dbg()
    big = Buf(_sent(1 << 16))
    out = Buf(_sent(1 << 16))
    sw, mean, std = I3(2, 1, 0), D3(1.0, 2.0, 3.0), D3(1.0, 1.0, 1.0)

    def bytes_(n_floats, off=0):
        return (vp(big.ptr + off), 4 * n_floats)

    def obytes(n_floats, off=0):
        return (vp(out.ptr + off), 4 * n_floats)
    act = L.cdiv(9, 8) * L.act_hp(5) * L.act_wp(7) * 8
    # name -> (call with keyword overrides, the in / out footprints in floats, the buffers' names, a shape that is refused)
    entries = {
        "nchw_to_c8p": (lambda i, o, C_=9: d.mpn_debug_nchw_to_c8p(*i, C_, 5, 7, *o), 9 * 35, act, "d_in", "d_out"),
        "c8p_to_nchw": (lambda i, o, C_=9: d.mpn_debug_c8p_to_nchw(*i, C_, 5, 7, *o), act, 9 * 35, "d_in", "d_out"),
        "rowmajor_to_c8": (lambda i, o, C_=9: d.mpn_debug_rowmajor_to_c8(*i, 3, C_, *o), 27, 2 * 128 * 8, "d_x", "d_c8"),
        "c8_to_rowmajor": (lambda i, o, C_=9: d.mpn_debug_c8_to_rowmajor(*i, 3, C_, *o), 2 * 128 * 8, 27, "d_c8", "d_y"),
        "unpack_pooled": (lambda i, o, C_=9: d.mpn_debug_unpack_pooled(*i, 3, C_, 4, 5, *o), 2 * 4 * 5 * 8, 3 * 9 * 4, "d_xc8", "d_out"),
        "copy_cols": (lambda i, o, C_=9: d.mpn_debug_copy_cols(*i, C_, 2, 3, 4 if C_ else 0, *o), 2 * 9 + 6, 12, "d_src", "d_dst"),
        "pack_conv_weights_first": (lambda i, o, C_=3: d.mpn_debug_pack_conv_weights_first(*i, C_, 5, *o), 5 * 3 * 9, 36 * 128, "d_w", "d_w36"),
        "maxpool2x2_c8p": (lambda i, o, C_=9: d.mpn_debug_maxpool2x2_c8p(*i, C_, 5, 7, *o), act, 2 * L.act_hp(3) * L.act_wp(4) * 8, "d_in", "d_out"),
        "image_transform_c8p": (lambda i, o, C_=5: d.mpn_debug_image_transform_c8p(*i, C_, 7, sw, 1.0, mean, std, 0, 0, C_, 7, *o), 3 * 35, act // 2, "d_in", "d_out"),
        "image_transform_c8i": (lambda i, o, C_=5: d.mpn_debug_image_transform_c8i(*i, C_, 7, sw, 1.0, mean, std, 0, 0, *o, *NULLB), 3 * 35, 35 * 8, "d_in", "d_img"),
        "c8i_to_pixel_major": (lambda i, o, C_=9: d.mpn_debug_c8i_to_pixel_major(*i, C_, 5, 7, *o), 2 * 128 * 8, 35 * 16, "d_c8i", "d_pm"),
        "im2col3_c8i": (lambda i, o, C_=5: d.mpn_debug_im2col3_c8i(*i, C_, 7, 3, 3, 1, 1, *o), 3 * 35, 8 * 128 * 8, "d_img", "d_col"),
        "permute_w3": (lambda i, o, C_=5: d.mpn_debug_permute_w3(*i, C_, 9, *o), 5 * 27, 5 * 27, "d_w", "d_o"),
        "c8i_c8p": (lambda i, o, C_=9: d.mpn_debug_c8i_c8p(*i, *o, C_, 5, 7, 1), 2 * 128 * 8, act, "d_c8i", "d_c8p"),
        "c8i_mosaic": (lambda i, o, C_=9: d.mpn_debug_c8i_mosaic(*i, *o, C_, 2, 3, 5, 7, 2, 1), 2 * 128 * 8, 2 * L.act_hp(12) * L.act_wp(16) * 8, "d_c8i", "d_mos"),
    }
    # the alignment each buffer's accesses need (layout_debug.h): 16 bytes where the kernel moves float4 records, 4 otherwise
    vec_in = {"maxpool2x2_c8p", "c8i_to_pixel_major", "c8i_c8p", "c8i_mosaic"}
    vec_out = {"nchw_to_c8p", "rowmajor_to_c8", "maxpool2x2_c8p", "image_transform_c8p", "image_transform_c8i", "c8i_to_pixel_major", "im2col3_c8i", "c8i_c8p",
               "c8i_mosaic"}
    for name, (call, n_in, n_out, in_name, out_name) in entries.items():
        _ok(call(bytes_(n_in), obytes(n_out)))                       # the exact footprints are accepted
        torch.cuda.synchronize()
        out2 = Buf(_sent(1 << 16))                                   # (a fresh output for the refusals below)

        def ob2(n_floats, off=0):
            return (vp(out2.ptr + off), 4 * n_floats)
        _invalid(call(NULLB, ob2(n_out)))
        _invalid(call(bytes_(n_in), NULLB))
        _short(call((vp(big.ptr), 4 * n_in - 1), ob2(n_out)), in_name)
        _short(call(bytes_(n_in), (vp(out2.ptr), 4 * n_out - 1)), out_name)
        _invalid(call(bytes_(n_in), ob2(n_out), C_=0))
        _misaligned(call(bytes_(n_in, off=2), ob2(n_out)), in_name)
        _misaligned(call(bytes_(n_in), ob2(n_out, off=2)), out_name)
        if name in vec_in:
            _misaligned(call(bytes_(n_in, off=4), ob2(n_out)), in_name)
        if name in vec_out:
            _misaligned(call(bytes_(n_in), ob2(n_out, off=8)), out_name)
        assert _is_sent(out2.read()), name + ": a refused call wrote something"
    # shapes outside an entry's own checks
    o = Buf(_sent(1 << 16))
    ob = B(o)
    ib = B(big)
    _invalid(d.mpn_debug_unpack_pooled(*ib, 6, 9, 4, 5, *ob))                       # Mp < N
    _invalid(d.mpn_debug_copy_cols(*ib, 5, 2, 3, 4, *ob))                           # ld < col0 + ncols
    _invalid(d.mpn_debug_copy_cols(*ib, 9, -1, 3, 4, *ob))
    _invalid(d.mpn_debug_pack_conv_weights_first(*ib, 5, 5, *ob))                   # Cin > 4
    _invalid(d.mpn_debug_image_transform_c8p(*ib, 5, 7, I3(0, 1, 3), 1.0, mean, std, 0, 0, 5, 7, *ob))   # a plane index outside 0..2
    _invalid(d.mpn_debug_image_transform_c8p(*ib, 5, 7, I3(-1, 1, 2), 1.0, mean, std, 0, 1, 5, 7, *ob))
    _invalid(d.mpn_debug_image_transform_c8p(*ib, 5, 7, sw, 1.0, mean, std, 0, 0, 6, 7, *ob))            # the plain form on a larger canvas
    _invalid(d.mpn_debug_image_transform_c8p(*ib, 5, 7, sw, 1.0, mean, std, 0, 1, 4, 7, *ob))            # a canvas smaller than the image
    _invalid(d.mpn_debug_image_transform_c8i(*ib, 5, 7, I3(0, 3, 1), 1.0, mean, std, 0, 0, *ob, *NULLB))
    _invalid(d.mpn_debug_im2col3_c8i(*ib, 2, 2, 7, 7, 1, 0, *ob))                   # a kernel larger than the padded image
    _invalid(d.mpn_debug_c8i_mosaic(*ib, *ob, 8, 4, 3, 5, 7, 2, 1))                 # cap < N
    _invalid(d.mpn_debug_pack_conv_weights(*ib, *NULLB, 0, 5, *ob, *ob))
    _short(d.mpn_debug_pack_conv_weights(*ib, *NULLB, 3, 5, *ob, vp(o.ptr), 4 * 127), "d_bpk")
    _short(d.mpn_debug_pack_conv_weights(*ib, vp(big.ptr), 4 * 4, 3, 5, *ob, *ob), "d_b")
    _short(d.mpn_debug_pack_conv_graph(*ib, *NULLB, 3, 5, 9, 1, vp(o.ptr), 9 * 2 * 128 * 8 * 2 - 1, *NULLB), "d_wpk")
    _short(d.mpn_debug_pack_conv_graph(*ib, *NULLB, 3, 5, 9, 0, vp(o.ptr), 9 * 128 * 8 * 4 - 1, *ob), "d_wpk")
    _invalid(d.mpn_debug_pack_conv_graph(*ib, *NULLB, 3, 5, 9, 0, *ob, *NULLB))     # the fp32 form needs d_bpk
    _invalid(d.mpn_debug_shard_pack_rows(*ib, *ib, 5, 2, 2, 1, 3, *ob))             # rank >= world
    _invalid(d.mpn_debug_shard_pack_rows(*NULLB, *NULLB, 5, 2, 0, 1, 3, *ob))       # a rank that owns rows needs its tables
    _short(d.mpn_debug_shard_pack_rows(*ib, *ib, 5, 2, 0, 1, 3, vp(o.ptr), 4 * 45 - 1), "d_rec")
    _short(d.mpn_debug_shard_unpack_rows(vp(big.ptr), 4 * 90 - 1, 5, 2, 1, 3, *ob, *ob), "d_all")
    _invalid(d.mpn_debug_shard_unpack_rows(*ib, 0, 2, 1, 3, *ob, *ob))
    _short(d.mpn_debug_shard_pack_classes(*ib, *ib, *ib, *NULLB, 5, 2, 0, 64, vp(o.ptr), 4 * 3 * (1 + 64 * 6) - 1), "d_rec")
    _short(d.mpn_debug_shard_pack_classes(*ib, *ib, *ib, *ib, 5, 2, 0, 64, vp(o.ptr), 4 * 3 * (1 + 64 * 11) - 1), "d_rec")
    _invalid(d.mpn_debug_shard_pack_classes(*ib, *ib, *ib, *NULLB, 5, 2, 2, 64, *ob))
    _short(d.mpn_debug_shard_unpack_classes(vp(big.ptr), 4 * 2 * 3 * (1 + 64 * 6) - 1, 5, 2, 64, *ob, *ob, *ob, *NULLB), "d_all")
    _invalid(d.mpn_debug_shard_unpack_classes(*ib, 5, 0, 64, *ob, *ob, *ob, *NULLB))
    # the halo entry: a short map, a misaligned map, a null map, a non-positive dimension — none launches
    p1, n1 = (vp * 1)(o.ptr), (cs * 1)(4 * act)
    one = lambda v: (ci * 1)(v)  # noqa: E731
    _short(d.mpn_debug_c8p_zero_halos(1, p1, (cs * 1)(4 * act - 1), one(9), one(5), one(7)), "d_map")
    _misaligned(d.mpn_debug_c8p_zero_halos(1, (vp * 1)(o.ptr + 8), n1, one(9), one(5), one(7)), "d_map")
    _invalid(d.mpn_debug_c8p_zero_halos(1, (vp * 1)(None), n1, one(9), one(5), one(7)))
    _invalid(d.mpn_debug_c8p_zero_halos(1, p1, n1, one(9), one(0), one(7)))
    _invalid(d.mpn_debug_c8p_zero_halos(-1, p1, n1, one(9), one(5), one(7)))
    _invalid(d.mpn_debug_c8p_zero_halos(1, None, n1, one(9), one(5), one(7)))
    # a second map refused after a first one was accepted: still nothing launched
    p2 = (vp * 2)(o.ptr, o.ptr + 4 * act)
    two = lambda a, b: (ci * 2)(a, b)  # noqa: E731
    _short(d.mpn_debug_c8p_zero_halos(2, p2, (cs * 2)(4 * act, 4 * act - 4), two(9, 9), two(5, 5), two(7, 7)), "d_map")
    # the two public entries
    _invalid(d.mpn_maxpool2x2_ceil_forward(None, 3, 5, 7, vp(o.ptr), None))
    _invalid(d.mpn_maxpool2x2_ceil_forward(vp(big.ptr), 3, 0, 7, vp(o.ptr), None))
    _invalid(d.mpn_pack_det_record(vp(big.ptr), vp(big.ptr), 0, vp(o.ptr), None))
    _invalid(d.mpn_pack_det_record(vp(big.ptr), None, 5, vp(o.ptr), None))
    assert _is_sent(o.read()), "a refused call wrote something"
    assert _is_sent(big.read())
