"""Every launch form of the VGG trunk's 3x3 convolution (dense.hip: conv3x3_c8p, conv3x3_first_c8p, maxpool2x2_c8p) against a float64
convolution computed on the host.

The forms are reached one at a time through mpn_debug_conv3x3_form (debug flavour only): the weights go through the real packers, the input
is laid out by nchw_to_c8p into a zeroed C8P buffer (a zero input halo is the contract), and ONE call writes the raw C8P output buffers this
file owns, pre-filled with a sentinel NaN and read back raw.  Three output modes: the full map, the pooled map only (out.p == nullptr) and
both (a tap layer).  Every run asserts the plan that was launched (mpn_debug_conv3x3_last_plan, written after the dispatcher's clamps):
(variant, wino_tc, splits, chunks_per_split, tail_first, tail_splits, tail_cps, reduce kernel ran), so a clamped split or a changed cost
model cannot quietly send a case to another kernel.  A new trunk kernel adds rows to CASES.  Four tiers:
  * exact: operands are integers, |x| <= 2, |w| <= 2, |b| <= 8.  The direct kernels' partial sums are integers of magnitude
    <= 9 Cin 4 + 8 < 2^24.  Winograd F(2x2,3x3): G g G^T holds multiples of 1/4 of magnitude <= 9/4 2, B^T d B integers <= 4 2, so every
    product, every partial sum over the input channels and every term of A^T M A is a multiple of 1/4 of magnitude
    <= 9 (Cin 9/4 2 4 2) + 8 = 324 Cin + 8 <= 165 896 < 2^22 for Cin <= 512: exact in fp32 in any order, split or not.  Each form equals
    float64 bit for bit, full map and pooled map; outside the H x W interior of every plane the sentinel survives (no halo / pitch write);
    the pad lanes of the last channel block are +0.0; the buffer a mode does not ask for is untouched;
  * accuracy: He-scaled weights on non-negative, mixed-sign and wide-range activations; e = max |y - y64| / (sum |x w| + |b|) against the
    same figure of the oracle's sequential fp32 chain (O.conv3x3, floored at 2^-24), within ACC_FACTOR of it; the pooled map the same way
    against the float64 pooled map (the denominator pooled by max, which bounds the pooled error of a correct pool);
  * edge: +-inf, NaN, +-1e30 and subnormals at corners, on borders, in the first / last channel; a subnormal and a huge weight.  Direct forms
    and the first-layer kernel: every output's class equals the elementwise float64 sum's; Winograd: a non-finite input reaches only the
    outputs whose 2x2 tile's 4x4 input patch holds it, every other output keeps its bits.  ReLU(NaN) follows RELU_NAN per family (what
    include/mpn.h states), reduce-kernel tiles included; a pooling window ignores its NaNs and a window of NaNs gives -inf in every kernel
    that pools;
  * invariance: bit-identical run to run and whatever ran before on the stream (stale split-K slabs); split / tail split equal the
    unsplit form bit for bit on the exact operands and within fp32 reassociation otherwise; the fused pool equals maxpool2x2_c8p of the same
    form's full map; batch_invariant gives a map the same bits at any height of a taller canvas.

Measured on the MI355X (accuracy tier, e over the oracle chain's e, min - max over the three data sets and the cases of a form; full map,
then pooled map): direct unsplit 0.63-1.31 / 0.63-1.35, direct split-K 0.25-0.72 / 0.24-0.60, first-layer kernel 0.89-1.15;
Winograd 16 x 16 blocks: unsplit 0.47-1.22 / 0.46-0.49, uniform split 0.21-0.42 / 0.23-0.29, tail split 0.27-1.00 / 0.31-0.56;
8 x 32 blocks: unsplit 0.36-0.85 / 0.30-0.47, uniform split 0.15-0.35 / 0.14-0.35, tail split 0.36-1.13 / 0.31-0.48; batch_invariant
0.45-0.67 / 0.31-0.42.  At 512 input channels (never measured before): unsplit 0.37-0.55, uniform split 0.14-0.22, tail split 0.38-0.68,
batch_invariant 0.34-0.45 (the chain's error grows with K, the MFMA's chunked sums less so).  Default dispatch on the VGG-16 shapes
(non-negative data): conv1_1 0.94, conv1_2 0.30, conv2_2 0.23, conv3_3 0.29, conv4_3 0.28, conv5_x 0.20.  No form needs a factor of its
own: 1.5 (direct) and 2.0 (Winograd) hold everywhere.
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KNOB_DEFAULTS = dict(conv_variant=0, conv_split=0, wino_tc=0)
SENT = 0x7FA5A5A5
CONV, FIRST, POOL = 0, 1, 2
FULL, POOLED, BOTH = "full", "pool", "both"
ALL_MODES = (FULL, POOLED, BOTH)


def _c(kind, Cin, H, W, Cout, plan, variant=0, split=0, tc=0, bi=0, wino=None, modes=None):
    """plan = (variant, wino_tc, splits, chunks_per_split, tail_first, tail_splits, tail_cps, reduce ran); variant 36 = the K = 36 first-layer
    kernel, -1 = maxpool2x2_c8p.  wino: the Winograd packing is passed beside the direct one (the trunk does from 16 input channels on)"""
    if wino is None:
        wino = int(variant == 7 or (variant == 0 and Cin >= 16))
    if modes is None:
        modes = ALL_MODES if kind == CONV else ((FULL,) if kind == FIRST else (POOLED,))
    return dict(kind=kind, Cin=Cin, H=H, W=W, Cout=Cout, plan=tuple(plan), knobs=dict(conv_variant=variant, conv_split=split, wino_tc=tc),
                bi=bi, wino=wino, modes=modes)


# name: direct variants d1..d6 (1 / 3: 128 couts x 4 rows x 32 columns, 2 / 4: 64 x 8 x 32, 5: 128 x 8 x 32, 6: 64 x 16 x 32), _s = uniform
# split-K; Winograd w8 (16 x 16 px blocks) / w16 (8 x 32 px), _s = uniform split, _t = tail split, wbi = batch_invariant; first = K = 36
# kernel; pool = maxpool2x2_c8p; vgg = the default dispatch (every knob at its default) on the VGG-16 layer shapes of a 600 x 1000 image.
CASES = {
    "d1_c3_5x33_o129": _c(CONV, 3, 5, 33, 129, (1, 0, 1, 1, 0, 0, 0, 0), variant=1, split=1),
    "d1_c24_4x32_o7": _c(CONV, 24, 4, 32, 7, (1, 0, 1, 3, 0, 0, 0, 0), variant=1, split=1),
    "d1_c9_1x1_o8": _c(CONV, 9, 1, 1, 8, (1, 0, 1, 2, 0, 0, 0, 0), variant=1, split=1),
    "d2_c8_9x31_o65": _c(CONV, 8, 9, 31, 65, (2, 0, 1, 1, 0, 0, 0, 0), variant=2, split=1),
    "d2_c9_7x17_o63": _c(CONV, 9, 7, 17, 63, (2, 0, 1, 2, 0, 0, 0, 0), variant=2, split=1),
    "d2_c8_1x37_o65": _c(CONV, 8, 1, 37, 65, (2, 0, 1, 1, 0, 0, 0, 0), variant=2, split=1),
    "d3_c9_3x15_o200": _c(CONV, 9, 3, 15, 200, (3, 0, 1, 2, 0, 0, 0, 0), variant=3, split=1),
    "d3_c24_5x33_o128": _c(CONV, 24, 5, 33, 128, (3, 0, 1, 3, 0, 0, 0, 0), variant=3, split=1),
    "d4_c24_8x16_o64": _c(CONV, 24, 8, 16, 64, (4, 0, 1, 3, 0, 0, 0, 0), variant=4, split=1),
    "d4_c3_9x33_o1": _c(CONV, 3, 9, 33, 1, (4, 0, 1, 1, 0, 0, 0, 0), variant=4, split=1),
    "d5_c8_17x33_o128": _c(CONV, 8, 17, 33, 128, (5, 0, 1, 1, 0, 0, 0, 0), variant=5, split=1),
    "d5_c24_7x31_o129": _c(CONV, 24, 7, 31, 129, (5, 0, 1, 3, 0, 0, 0, 0), variant=5, split=1),
    "d6_c24_15x47_o8": _c(CONV, 24, 15, 47, 8, (6, 0, 1, 3, 0, 0, 0, 0), variant=6, split=1),
    "d6_c9_17x32_o65": _c(CONV, 9, 17, 32, 65, (6, 0, 1, 2, 0, 0, 0, 0), variant=6, split=1),
    "d6_c8_16x32_o1": _c(CONV, 8, 16, 32, 1, (6, 0, 1, 1, 0, 0, 0, 0), variant=6, split=1),
    "d1_s2_c96_5x33_o129": _c(CONV, 96, 5, 33, 129, (1, 0, 2, 6, 0, 0, 0, 1), variant=1, split=2),
    "d1_s3_c100_9x17_o7": _c(CONV, 100, 9, 17, 7, (1, 0, 3, 5, 0, 0, 0, 1), variant=1, split=3),
    "d2_s3_c96_9x17_o65": _c(CONV, 96, 9, 17, 65, (2, 0, 3, 4, 0, 0, 0, 1), variant=2, split=3),
    "d3_s8_c128_7x31_o200": _c(CONV, 128, 7, 31, 200, (3, 0, 8, 2, 0, 0, 0, 1), variant=3, split=8),
    "d4_s2_c96_17x33_o63": _c(CONV, 96, 17, 33, 63, (4, 0, 2, 6, 0, 0, 0, 1), variant=4, split=2),
    "d5_s3_c96_9x15_o129": _c(CONV, 96, 9, 15, 129, (5, 0, 3, 4, 0, 0, 0, 1), variant=5, split=3),
    "d6_s8_c128_17x16_o7": _c(CONV, 128, 17, 16, 7, (6, 0, 8, 2, 0, 0, 0, 1), variant=6, split=8),
    "w8_c24_17x33_o65": _c(CONV, 24, 17, 33, 65, (7, 8, 1, 3, 0, 0, 0, 0), variant=7, split=1, tc=8),
    "w8_c9_15x15_o63": _c(CONV, 9, 15, 15, 63, (7, 8, 1, 2, 0, 0, 0, 0), variant=7, split=1, tc=8),
    "w8_c3_7x31_o200": _c(CONV, 3, 7, 31, 200, (7, 8, 1, 1, 0, 0, 0, 0), variant=7, split=1, tc=8),
    "w8_c8_1x1_o8": _c(CONV, 8, 1, 1, 8, (7, 8, 1, 1, 0, 0, 0, 0), variant=7, split=1, tc=8),
    "w8_c8_1x37_o1": _c(CONV, 8, 1, 37, 1, (7, 8, 1, 1, 0, 0, 0, 0), variant=7, split=1, tc=8),
    "w8_c24_16x32_o64": _c(CONV, 24, 16, 32, 64, (7, 8, 1, 3, 0, 0, 0, 0), variant=7, split=1, tc=8),
    "w8_c24_9x17_o129": _c(CONV, 24, 9, 17, 129, (7, 8, 1, 3, 0, 0, 0, 0), variant=7, split=1, tc=8),
    "w8_c512_17x33_o64": _c(CONV, 512, 17, 33, 64, (7, 8, 1, 64, 0, 0, 0, 0), variant=7, split=1, tc=8),
    "w8_s2_c96_17x33_o65": _c(CONV, 96, 17, 33, 65, (7, 8, 2, 6, 0, 0, 0, 1), variant=7, split=2, tc=8),
    "w8_s3_c100_9x31_o128": _c(CONV, 100, 9, 31, 128, (7, 8, 3, 5, 0, 0, 0, 1), variant=7, split=3, tc=8),
    "w8_s8_c128_15x16_o7": _c(CONV, 128, 15, 16, 7, (7, 8, 8, 2, 0, 0, 0, 1), variant=7, split=8, tc=8),
    "w8_s4_c512_17x33_o64": _c(CONV, 512, 17, 33, 64, (7, 8, 4, 16, 0, 0, 0, 1), variant=7, split=4, tc=8),
    "w16_c24_17x33_o65": _c(CONV, 24, 17, 33, 65, (7, 16, 1, 3, 0, 0, 0, 0), variant=7, split=1, tc=16),
    "w16_c9_15x15_o63": _c(CONV, 9, 15, 15, 63, (7, 16, 1, 2, 0, 0, 0, 0), variant=7, split=1, tc=16),
    "w16_c3_7x31_o200": _c(CONV, 3, 7, 31, 200, (7, 16, 1, 1, 0, 0, 0, 0), variant=7, split=1, tc=16),
    "w16_c8_1x1_o8": _c(CONV, 8, 1, 1, 8, (7, 16, 1, 1, 0, 0, 0, 0), variant=7, split=1, tc=16),
    "w16_c8_1x37_o1": _c(CONV, 8, 1, 37, 1, (7, 16, 1, 1, 0, 0, 0, 0), variant=7, split=1, tc=16),
    "w16_c24_16x32_o64": _c(CONV, 24, 16, 32, 64, (7, 16, 1, 3, 0, 0, 0, 0), variant=7, split=1, tc=16),
    "w16_c24_9x17_o129": _c(CONV, 24, 9, 17, 129, (7, 16, 1, 3, 0, 0, 0, 0), variant=7, split=1, tc=16),
    "w16_c512_17x33_o64": _c(CONV, 512, 17, 33, 64, (7, 16, 1, 64, 0, 0, 0, 0), variant=7, split=1, tc=16),
    "w16_s2_c96_17x33_o65": _c(CONV, 96, 17, 33, 65, (7, 16, 2, 6, 0, 0, 0, 1), variant=7, split=2, tc=16),
    "w16_s3_c100_9x31_o128": _c(CONV, 100, 9, 31, 128, (7, 16, 3, 5, 0, 0, 0, 1), variant=7, split=3, tc=16),
    "w16_s8_c128_15x16_o7": _c(CONV, 128, 15, 16, 7, (7, 16, 8, 2, 0, 0, 0, 1), variant=7, split=8, tc=16),
    "w16_s4_c512_17x33_o64": _c(CONV, 512, 17, 33, 64, (7, 16, 4, 16, 0, 0, 0, 1), variant=7, split=4, tc=16),
    "w8_t2_c24_40x40_o65": _c(CONV, 24, 40, 40, 65, (7, 8, 1, 3, 8, 2, 2, 1), variant=7, split=-2, tc=8),
    "w8_t3_c96_57x31_o64": _c(CONV, 96, 57, 31, 64, (7, 8, 1, 12, 4, 3, 4, 1), variant=7, split=-3, tc=8),
    "w8_t4_c512_33x33_o64": _c(CONV, 512, 33, 33, 64, (7, 8, 1, 64, 4, 4, 16, 1), variant=7, split=-4, tc=8),
    "w16_t2_c24_23x65_o129": _c(CONV, 24, 23, 65, 129, (7, 16, 1, 3, 12, 2, 2, 1), variant=7, split=-2, tc=16),
    "w16_t8_c128_31x33_o8": _c(CONV, 128, 31, 33, 8, (7, 16, 1, 16, 4, 8, 2, 1), variant=7, split=-8, tc=16),
    "w16_t4_c512_17x63_o64": _c(CONV, 512, 17, 63, 64, (7, 16, 1, 64, 3, 4, 16, 1), variant=7, split=-4, tc=16),
    "wbi_c64_7x7_o72": _c(CONV, 64, 7, 7, 72, (7, 16, 1, 8, 0, 0, 0, 0), variant=7, bi=1),
    "wbi_c24_41x15_o8": _c(CONV, 24, 41, 15, 8, (7, 16, 1, 3, 0, 0, 0, 0), variant=7, bi=1),
    "wbi_c512_41x33_o64": _c(CONV, 512, 41, 33, 64, (7, 16, 1, 64, 0, 0, 0, 0), variant=7, bi=1),
    # the K = 36 first-layer kernel (64-cout tiles, 8 rows x 32 columns, persistent over tiles)
    "first_c3_17x33_o72": _c(FIRST, 3, 17, 33, 72, (36, 0, 1, 1, 0, 0, 0, 0)),
    "first_c3_9x31_o200": _c(FIRST, 3, 9, 31, 200, (36, 0, 1, 1, 0, 0, 0, 0)),
    "first_c1_1x1_o7": _c(FIRST, 1, 1, 1, 7, (36, 0, 1, 1, 0, 0, 0, 0)),
    "first_c4_8x32_o64": _c(FIRST, 4, 8, 32, 64, (36, 0, 1, 1, 0, 0, 0, 0)),
    # maxpool2x2_c8p on its own
    "pool_c9_7x9": _c(POOL, 9, 7, 9, 9, (-1, 0, 0, 0, 0, 0, 0, 0)),
    "pool_c64_1x1": _c(POOL, 64, 1, 1, 64, (-1, 0, 0, 0, 0, 0, 0, 0)),
    "pool_c3_1x5": _c(POOL, 3, 1, 5, 3, (-1, 0, 0, 0, 0, 0, 0, 0)),
    "pool_c200_17x33": _c(POOL, 200, 17, 33, 200, (-1, 0, 0, 0, 0, 0, 0, 0)),
    "pool_c8_16x32": _c(POOL, 8, 16, 32, 8, (-1, 0, 0, 0, 0, 0, 0, 0)),
    # default dispatch, VGG-16 at 600 x 1000, in the output mode the trunk runs the layer in (run_trunk in pipeline.hip): conv1_1 on the
    # first-layer kernel; conv1_2 / conv2_2 / conv3_3 / conv4_3 with the fused pool, pooled map only; conv5_x full map
    "vgg_conv1_1": _c(FIRST, 3, 600, 1000, 64, (36, 0, 1, 1, 0, 0, 0, 0)),
    "vgg_conv1_2": _c(CONV, 64, 600, 1000, 64, (7, 8, 1, 8, 0, 0, 0, 0), modes=(POOLED,)),
    "vgg_conv2_2": _c(CONV, 128, 300, 500, 128, (7, 8, 1, 16, 0, 0, 0, 0), modes=(POOLED,)),
    "vgg_conv3_3": _c(CONV, 256, 150, 250, 256, (7, 16, 1, 32, 512, 2, 16, 1), modes=(POOLED,)),
    "vgg_conv4_3": _c(CONV, 512, 75, 125, 512, (7, 8, 1, 64, 256, 4, 16, 1), modes=(POOLED,)),
    "vgg_conv5_x": _c(CONV, 512, 38, 63, 512, (7, 16, 3, 22, 0, 0, 0, 1), modes=(FULL,)),
}
VGG = [n for n in CASES if n.startswith("vgg_")]
SMALL = [n for n in CASES if n not in VGG]
CONVS = [n for n in SMALL if CASES[n]["kind"] == CONV]
SPLITS = [n for n in CONVS if CASES[n]["plan"][7]]   # every case that finishes in conv_splitk_reduce_kernel
# ReLU(NaN) per family (include/mpn.h, convolution edge values): NaN on the direct forms and the first-layer kernel (t < 0 ? 0 : t), 0 on
# every Winograd launch, the tiles the reduce kernel finishes included
RELU_NAN = {1: np.nan, 2: np.nan, 3: np.nan, 4: np.nan, 5: np.nan, 6: np.nan, 36: np.nan, 7: 0.0}
# largest e(form) / e(oracle fp32 chain) allowed: the project's factors (test_gpu_conv_numerics.py: 1.5 direct fp32, 2.0 Winograd)
ACC_FACTOR = {"direct": 1.5, "wino": 2.0}


def _family(name):
    return "wino" if CASES[name]["plan"][0] == 7 else "direct"


@functools.lru_cache(maxsize=None)
def _dbg():
    from multipathnet_amd import _lib
    lib = _lib.load("debug")
    vp, i = C.c_void_p, C.c_int
    lib.mpn_debug_conv3x3_form.argtypes = [vp, i, i, i, vp, vp, i, i, i, i, i, vp, vp]
    lib.mpn_debug_act_elems.restype = C.c_size_t
    lib.mpn_debug_act_elems.argtypes = [i, i, i, C.POINTER(i), C.POINTER(i)]
    lib.mpn_debug_conv3x3_last_plan.restype = None
    return lib


@contextlib.contextmanager
def _knobs(lib, **kv):
    for k, v in kv.items():
        getattr(lib, "mpn_debug_set_" + k)(v)
    try:
        yield
    finally:
        for k in kv:
            getattr(lib, "mpn_debug_set_" + k)(KNOB_DEFAULTS[k])


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.device("cuda", 0)) if a is not None else None


class Raw(object):
    """a raw C8P buffer [Cb][Hp][Wp][8] read back as uint32 words"""

    def __init__(self, words, C_, H, W, Hp, Wp):
        self.C, self.H, self.W = C_, H, W
        self.w = words.reshape((C_ + 7) // 8, Hp, Wp, 8)

    def interior(self):
        """[C, H, W] float32"""
        v = self.w[:, 1:self.H + 1, 1:self.W + 1, :].transpose(0, 3, 1, 2).reshape(-1, self.H, self.W)
        return np.ascontiguousarray(v[:self.C]).view(np.float32)

    def outside_untouched(self):
        """words outside the H x W interior of every plane that no longer hold the sentinel"""
        m = self.w != SENT
        m[:, 1:self.H + 1, 1:self.W + 1, :] = False
        return int(m.sum())

    def pad_lanes(self):
        """the channels past C in the last block, interior pixels (uint32 words)"""
        return self.w[-1, 1:self.H + 1, 1:self.W + 1, self.C - (self.w.shape[0] - 1) * 8:]


def _sentinel_buf(lib, C_, H, W):
    hp, wp = C.c_int(0), C.c_int(0)
    n = lib.mpn_debug_act_elems(C_, H, W, C.byref(hp), C.byref(wp))
    assert n == (C_ + 7) // 8 * hp.value * wp.value * 8
    t = torch.full((n,), SENT, dtype=torch.int32, device=torch.device("cuda", 0))
    return t, hp.value, wp.value


def last_plan():
    p = (C.c_int * 8)()
    _dbg().mpn_debug_conv3x3_last_plan(p)
    return tuple(p)


def run(name, x, w=None, b=None, relu=0, mode=None, knobs=None, plan=None, bi=None):
    """ONE launch of case `name` on operands x [Cin,H,W], w [Cout,Cin,3,3], b [Cout]; returns (full, pooled) as Raw (None where the mode
    does not ask for the buffer).  Asserts the launched plan (`plan` overrides the table's when `knobs` / `bi` do), and that the buffer the
    mode does not ask for still holds the sentinel everywhere."""
    from multipathnet_amd import _lib
    c = CASES[name]
    lib = _dbg()
    mode = mode or c["modes"][0]
    Cin, H, W = x.shape
    Cout = Cin if c["kind"] == POOL else w.shape[0]
    PH, PW = (H + 1) // 2, (W + 1) // 2
    fbuf, fhp, fwp = _sentinel_buf(lib, Cout, H, W)
    pbuf, php, pwp = _sentinel_buf(lib, Cout, PH, PW)
    xd, wd, bd = _dev(x), _dev(w), _dev(b)
    want_f, want_p = mode in (FULL, BOTH), mode in (POOLED, BOTH)
    torch.cuda.synchronize()
    with _knobs(lib, **dict(c["knobs"], **(knobs or {}))):
        rc = lib.mpn_debug_conv3x3_form(_ptr(xd), Cin, H, W, _ptr(wd), _ptr(bd), Cout, int(relu), c["kind"], c["wino"],
                                        int(c["bi"] if bi is None else bi), _ptr(fbuf) if want_f else None, _ptr(pbuf) if want_p else None)
    if rc != 0:
        raise _lib.MpnError("mpn_debug_conv3x3_form(%s, %s) failed (%d): %s" % (name, mode, rc, lib.mpn_last_error().decode()))
    want = c["plan"] if plan is None and knobs is None and bi is None and (Cin, H, W, Cout) == (c["Cin"], c["H"], c["W"], c["Cout"]) else plan
    if want is not None:
        assert last_plan() == tuple(want), "%s (%s) launched plan %s, meant %s" % (name, mode, last_plan(), tuple(want))
    full = Raw(fbuf.cpu().numpy().view(np.uint32), Cout, H, W, fhp, fwp)
    pooled = Raw(pbuf.cpu().numpy().view(np.uint32), Cout, PH, PW, php, pwp)
    if not want_f:
        assert (full.w == SENT).all(), "%s (%s): the full-map buffer was written" % (name, mode)
    if not want_p:
        assert (pooled.w == SENT).all(), "%s (%s): the pooled buffer was written" % (name, mode)
    return (full if want_f else None), (pooled if want_p else None)


# ---------------------------------------------------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------------------------------------------------
def ref64(x, w, b=None, relu=0, absolute=False):
    xt, wt = torch.from_numpy(np.asarray(x, np.float64))[None], torch.from_numpy(np.asarray(w, np.float64))
    bt = torch.from_numpy(np.asarray(b, np.float64)) if b is not None else None
    if absolute:
        xt, wt, bt = xt.abs(), wt.abs(), (bt.abs() if bt is not None else None)
    Cin, H, W = xt.shape[1:]
    xp = torch.nn.functional.pad(xt, (1, 1, 1, 1))
    rows = max(1, 40000000 // (Cin * 9 * W))   # in strips of rows: the unfolded operand of a 600 x 1000 map would take gigabytes
    y = torch.cat([torch.nn.functional.conv2d(xp[:, :, y0:y0 + rows + 2], wt, bt) for y0 in range(0, H, rows)], 2)[0].numpy() + 0.0
    if relu and not absolute:
        y = np.where(y < 0, 0.0, y)
    return y


def pool_ref(y):
    """ceil-mode 2x2 max as the oracle takes it (v > m from -inf): NaNs of a window are ignored, a window of NaNs gives -inf"""
    Cc, H, W = y.shape
    p = np.full((Cc, (H + 1) // 2 * 2, (W + 1) // 2 * 2), -np.inf, y.dtype)
    p[:, :H, :W] = np.where(np.isnan(y), -np.inf, y)
    return p.reshape(Cc, (H + 1) // 2, 2, (W + 1) // 2, 2).max(axis=(2, 4))


def ref_elementwise(x, w, b=None):
    """float64 as an explicit sum of elementwise products (0 * inf = NaN, as the kernels compute it; no BLAS)"""
    Cin, H, W = x.shape
    Cout = w.shape[0]
    xt = torch.from_numpy(np.asarray(x, np.float64))[None]
    cols = torch.nn.functional.unfold(xt, (3, 3), padding=1)[0].numpy()  # [Cin * 9, H * W] (the zero padding multiplies like the zero halo)
    wf = np.asarray(w, np.float64).reshape(Cout, -1)
    y = np.zeros((Cout, H * W))
    with np.errstate(invalid="ignore", over="ignore"):
        for c0 in range(0, Cout, 16):
            y[c0:c0 + 16] = (wf[c0:c0 + 16, :, None] * cols[None, :, :]).sum(1)
        y = y.reshape(Cout, H, W)
        if b is not None:
            y = y + np.asarray(b, np.float64)[:, None, None]
    return y


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------------------------
def _seed(name, salt):
    return (sum((i + 1) * ord(ch) for i, ch in enumerate(name)) * 7919 + salt) % (2 ** 32)


def exact_operands(name, salt=0):
    """integers |x| <= 2, |w| <= 2, |b| <= 8 (the docstring's bound); random, so asymmetric in tap, cin and cout; pool cases: |x| <= 50"""
    c = CASES[name]
    rng = np.random.default_rng(_seed(name, 11 + salt))
    if c["kind"] == POOL:
        return rng.integers(-50, 51, (c["Cin"], c["H"], c["W"])).astype(np.float32), None, None
    x = rng.integers(-2, 3, (c["Cin"], c["H"], c["W"])).astype(np.float32)
    w = rng.integers(-2, 3, (c["Cout"], c["Cin"], 3, 3)).astype(np.float32)
    b = rng.integers(-8, 9, c["Cout"]).astype(np.float32)
    return x, w, b


def acc_operands(name, kind, salt=0):
    c = CASES[name]
    rng = np.random.default_rng(_seed(name, 101 + salt))
    x = rng.standard_normal((c["Cin"], c["H"], c["W"])).astype(np.float32)
    if kind == "nonneg":
        x = np.abs(x)
    elif kind == "wide":
        x = (x * np.exp2(rng.uniform(-12, 12, x.shape))).astype(np.float32)
    if c["kind"] == POOL:
        return x, None, None
    w = (rng.standard_normal((c["Cout"], c["Cin"], 3, 3)) * np.sqrt(2.0 / (c["Cin"] * 9))).astype(np.float32)
    b = (rng.standard_normal(c["Cout"]) * 0.1).astype(np.float32)
    return x, w, b


# ---------------------------------------------------------------------------------------------------------------------------------------
# tier 1: exact
# ---------------------------------------------------------------------------------------------------------------------------------------
def _check_layout(name, mode, raw, what):
    n = raw.outside_untouched()
    assert n == 0, "%s (%s): %d words of the %s buffer outside the H x W interior were written (halo / pitch padding)" % (name, mode, n, what)
    pl = raw.pad_lanes()
    assert (pl == 0).all(), "%s (%s): %d pad lanes of the %s map's last channel block are not +0.0" % (name, mode, int((pl != 0).sum()), what)


def _check_exact(name, mode, full, pooled, y64):
    if full is not None:
        y = full.interior()
        bad = _bits(y) != _bits(y64)
        assert not bad.any(), "%s (%s): %d outputs differ from float64, max |d| %g" % (name, mode, int(bad.sum()), np.abs(y - y64).max())
        _check_layout(name, mode, full, "full")
    if pooled is not None:
        p, p64 = pooled.interior(), pool_ref(y64)
        bad = _bits(p) != _bits(p64)
        assert not bad.any(), "%s (%s): %d pooled outputs differ from float64, max |d| %g" % (name, mode, int(bad.sum()), np.abs(p - p64).max())
        _check_layout(name, mode, pooled, "pooled")


@pytest.mark.parametrize("name", SMALL)
def test_exact(dev, name):
    """bit-exact against float64 in every output mode and epilogue; no write outside the interior; pad lanes +0.0"""
    c = CASES[name]
    x, w, b = exact_operands(name)
    if c["kind"] == POOL:
        _, pooled = run(name, x)
        _check_exact(name, POOLED, None, pooled, x.astype(np.float64))
        return
    for hb, relu in ((True, 0), (False, 1), (True, 1)):
        bb = b if hb else None
        y64 = ref64(x, w, bb, relu)
        for mode in c["modes"]:
            full, pooled = run(name, x, w, bb, relu, mode)
            _check_exact(name, "%s, bias %d, relu %d" % (mode, hb, relu), full, pooled, y64)


@pytest.mark.parametrize("name", VGG)
def test_exact_vgg_default_dispatch(dev, name):
    """the default dispatch on the real VGG-16 layer shapes, in the trunk's own output mode: the recorded plan, bit-exact, layout intact"""
    c = CASES[name]
    x, w, b = exact_operands(name)
    y64 = ref64(x, w, b, 1)
    full, pooled = run(name, x, w, b, 1, c["modes"][0])
    _check_exact(name, c["modes"][0], full, pooled, y64)


# ---------------------------------------------------------------------------------------------------------------------------------------
# tier 2: accuracy
# ---------------------------------------------------------------------------------------------------------------------------------------
ACC = ["d1_c24_4x32_o7", "d2_c9_7x17_o63", "d3_c24_5x33_o128", "d4_c24_8x16_o64", "d5_c24_7x31_o129", "d6_c24_15x47_o8",
       "d1_s3_c100_9x17_o7", "d2_s3_c96_9x17_o65", "d3_s8_c128_7x31_o200", "d4_s2_c96_17x33_o63", "d5_s3_c96_9x15_o129", "d6_s8_c128_17x16_o7",
       "w8_c24_17x33_o65", "w8_c512_17x33_o64", "w8_s2_c96_17x33_o65", "w8_s3_c100_9x31_o128", "w8_s4_c512_17x33_o64", "w8_t2_c24_40x40_o65",
       "w8_t3_c96_57x31_o64", "w8_t4_c512_33x33_o64",
       "w16_c24_17x33_o65", "w16_c512_17x33_o64", "w16_s2_c96_17x33_o65", "w16_s8_c128_15x16_o7", "w16_s4_c512_17x33_o64",
       "w16_t2_c24_23x65_o129", "w16_t8_c128_31x33_o8", "w16_t4_c512_17x63_o64", "wbi_c64_7x7_o72", "wbi_c512_41x33_o64",
       "first_c3_17x33_o72", "first_c3_9x31_o200"]


def _accuracy(name, kind, O, modes):
    c = CASES[name]
    x, w, b = acc_operands(name, kind)
    den = np.maximum(ref64(x, w, b, absolute=True), np.finfo(np.float32).tiny)
    fac = ACC_FACTOR[_family(name)]
    for mode in modes:
        relu = 0 if mode == FULL else 1   # pooled modes as the trunk runs them; the ReLU is 1-Lipschitz, the bound stands
        y64 = ref64(x, w, b, relu)
        yo = O.conv3x3(x, w, b, relu=bool(relu)).astype(np.float64)
        full, pooled = run(name, x, w, b, relu, mode)
        figs = []
        if full is not None:
            figs.append(("full", (np.abs(full.interior() - y64) / den).max(), (np.abs(yo - y64) / den).max()))
        if pooled is not None:
            pden = pool_ref(den)
            figs.append(("pooled", (np.abs(pooled.interior() - pool_ref(y64)) / pden).max(), (np.abs(pool_ref(yo) - pool_ref(y64)) / pden).max()))
        for what, e, e_orc in figs:
            e_orc = max(e_orc, 2.0 ** -24)
            print("ACC %s %s %s/%s ratio %.3f (e %.3g, oracle %.3g)" % (name, kind, mode, what, e / e_orc, e, e_orc))
        for what, e, e_orc in figs:
            e_orc = max(e_orc, 2.0 ** -24)
            assert e <= fac * e_orc, "%s/%s %s %s map: error %.3g is %.2fx the oracle chain's %.3g" % (name, kind, mode, what, e, e / e_orc, e_orc)


@pytest.mark.parametrize("kind", ["nonneg", "mixed", "wide"])
@pytest.mark.parametrize("name", ACC)
def test_accuracy(dev, O, name, kind):
    modes = CASES[name]["modes"]
    _accuracy(name, kind, O, modes if len(modes) == 1 else (FULL, BOTH))


@pytest.mark.parametrize("name", VGG)
def test_accuracy_vgg_default_dispatch(dev, O, name):
    """post-ReLU (non-negative) activations, what the trunk's layers really see"""
    _accuracy(name, "nonneg", O, CASES[name]["modes"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# tier 3: edge values
# ---------------------------------------------------------------------------------------------------------------------------------------
EDGE_DIRECT = ["d1_c3_5x33_o129", "d2_c8_9x31_o65", "d3_c24_5x33_o128", "d4_c24_8x16_o64", "d5_c24_7x31_o129", "d6_c9_17x32_o65",
               "d1_s2_c96_5x33_o129", "d2_s3_c96_9x17_o65", "d3_s8_c128_7x31_o200", "d4_s2_c96_17x33_o63", "d5_s3_c96_9x15_o129",
               "d6_s8_c128_17x16_o7", "first_c3_17x33_o72", "first_c3_9x31_o200"]
EDGE_WINO = ["w8_c24_17x33_o65", "w8_s2_c96_17x33_o65", "w8_s8_c128_15x16_o7", "w8_t2_c24_40x40_o65", "w8_t3_c96_57x31_o64",
             "w16_c24_17x33_o65", "w16_s3_c100_9x31_o128", "w16_t2_c24_23x65_o129", "w16_t8_c128_31x33_o8", "wbi_c24_41x15_o8"]


def _spots(Cin, H, W):
    """(channel, y, x, value): non-finite values at the four corners and on a border, in the first and the last channel"""
    return [(0, 0, 0, np.nan), (Cin - 1, H - 1, W - 1, np.inf), (0, 0, W - 1, -np.inf), (Cin - 1, H - 1, 0, np.nan), (0, H // 2, 0, np.inf)]


def edge_operands(name, salt=0):
    """returns x0 (finite: +-1e30 and subnormals planted), x (x0 + the non-finite spots), w (a subnormal first and a huge last weight), b"""
    c = CASES[name]
    Cin, H, W = c["Cin"], c["H"], c["W"]
    x0, w, b = acc_operands(name, "mixed", 7 + salt)
    mid = Cin // 2
    x0[mid, H // 2, W // 2] = 1.0e30
    x0[mid, 0, W // 2] = -1.0e30
    x0[Cin - 1, 0, W // 2 + 1] = 1.0e-40
    x0[0, H // 2, 1] = -3.0e-39
    x = x0.copy()
    for ch, yy, xx, v in _spots(Cin, H, W):
        x[ch, yy, xx] = v
    w[0, 0, 0, 0] = 1.0e-40
    w[-1, -1, -1, -1] = 1.0e20
    return x0, x, w, b


def _cls(a):
    return np.where(np.isnan(a), 0, np.where(a == np.inf, 1, np.where(a == -np.inf, 2, 3)))


@pytest.mark.parametrize("name", EDGE_DIRECT)
def test_edge_classes_direct(dev, name):
    """direct forms / first-layer kernel: every output's class (NaN, +inf, -inf, finite) is the elementwise float64 sum's; ReLU keeps NaN"""
    _, x, w, b = edge_operands(name)
    y64 = ref_elementwise(x, w, b)
    assert np.isnan(y64).any() and np.isinf(y64).any() and np.isfinite(y64).any()
    y = run(name, x, w, b, 0, FULL)[0].interior()
    bad = _cls(y) != _cls(y64)
    assert not bad.any(), "%s (no ReLU): %d outputs in the wrong class, e.g. %s vs %s" % (name, int(bad.sum()), y[bad][:4], y64[bad][:4])
    yr = run(name, x, w, b, 1, FULL)[0].interior()
    with np.errstate(invalid="ignore"):
        r64 = np.where(y64 < 0, 0.0, y64)   # t < 0 ? 0 : t: NaN passes (RELU_NAN)
    assert np.isnan(RELU_NAN[CASES[name]["plan"][0]])
    bad = _cls(yr) != _cls(r64)
    assert not bad.any(), "%s (ReLU): %d outputs in the wrong class, e.g. %s vs %s" % (name, int(bad.sum()), yr[bad][:4], r64[bad][:4])


def _wino_reach(Cin, H, W):
    """outputs a non-finite input may reach: those whose 2x2 tile's 4x4 input patch (rows ty - 1 .. ty + 2 of the tile at even ty) holds it"""
    m = np.zeros((H, W), bool)
    ty, tx = (np.arange(H) & ~1)[:, None], (np.arange(W) & ~1)[None, :]
    for _, iy, ix, _ in _spots(Cin, H, W):
        m |= (ty - 1 <= iy) & (iy <= ty + 2) & (tx - 1 <= ix) & (ix <= tx + 2)
    return m


@pytest.mark.parametrize("name", EDGE_WINO)
def test_edge_winograd(dev, name):
    """Winograd forms: a non-finite input spreads only over the outputs whose tile's input patch holds it, everything else keeps its bits;
    every non-finite float64 output is non-finite; ReLU(NaN) = 0 in EVERY launch of the family, reduce-kernel tiles included"""
    c = CASES[name]
    x0, x, w, b = edge_operands(name)
    y64 = ref_elementwise(x, w, b)
    reach = _wino_reach(c["Cin"], c["H"], c["W"])
    assert np.isnan(y64).any() and np.isinf(y64).any() and not reach.all()
    assert np.isfinite(y64[:, ~reach]).all()   # float64 itself keeps the planted values inside the reach
    y = run(name, x, w, b, 0, FULL)[0].interior()
    y0 = run(name, x0, w, b, 0, FULL)[0].interior()
    assert np.isfinite(y0).all()
    assert np.array_equal(_bits(y[:, ~reach]), _bits(y0[:, ~reach])), "%s: a non-finite input changed outputs outside its tiles' patches" % name
    assert not np.isfinite(y[~np.isfinite(y64)]).any(), "%s: a non-finite float64 output came out finite" % name
    assert np.isnan(y).any()
    assert RELU_NAN[7] == 0.0
    for mode in (FULL, BOTH):
        full, pooled = run(name, x, w, b, 1, mode)
        yr = full.interior()
        assert not np.isnan(yr).any(), "%s (%s): ReLU(NaN) must be 0 on every Winograd launch; %d NaN outputs" % (name, mode, int(np.isnan(yr).sum()))
        assert (yr[np.isnan(y)] == 0.0).all()
        assert np.array_equal(_bits(yr[:, ~reach]), _bits(np.where(y0 < 0, 0.0, y0)[:, ~reach]))
        if pooled is not None:
            assert np.array_equal(_bits(pooled.interior()), _bits(pool_ref(yr)))


POOL_RULE = ["d1_c3_5x33_o129", "d2_c8_9x31_o65", "d3_c24_5x33_o128", "d4_c24_8x16_o64", "d5_c24_7x31_o129", "d6_c9_17x32_o65",
             "d1_s2_c96_5x33_o129", "d2_s3_c96_9x17_o65", "d6_s8_c128_17x16_o7", "w8_c24_17x33_o65", "w8_s2_c96_17x33_o65", "w8_t2_c24_40x40_o65",
             "w16_c24_17x33_o65", "w16_s3_c100_9x31_o128", "w16_t2_c24_23x65_o129", "wbi_c24_41x15_o8"]


@pytest.mark.parametrize("name", POOL_RULE)
def test_edge_pool_rule(dev, name):
    """one pooling rule wherever the pool runs (fused in the direct kernel, fused in Winograd, in the reduce kernel): the NaNs of a window are
    ignored and a window of NaNs gives -inf, the oracle's v > m from -inf.  NaN inputs in every channel block make whole windows NaN, on the
    ceil-mode last row / column (odd H, W: one-element windows) too"""
    c = CASES[name]
    Cin, H, W = c["Cin"], c["H"], c["W"]
    x, w, b = acc_operands(name, "mixed", 3)
    x[0, min(3, H - 1), 3] = np.nan          # outputs rows 2..4 x columns 2..4 (direct): the window at (2..3, 2..3) is all NaN
    x[Cin - 1, H - 1, W - 1] = np.nan        # the last row / column
    x[0, H - 1, W // 2] = np.nan
    for relu in (0, 1):
        full, pooled = run(name, x, w, b, relu, BOTH)
        y, p = full.interior(), pooled.interior()
        want = pool_ref(y)
        assert not np.isnan(p).any(), "%s (relu %d): %d pooled outputs are NaN" % (name, relu, int(np.isnan(p).sum()))
        assert np.array_equal(_bits(p), _bits(want)), "%s (relu %d): fused pool differs from the rule on %d outputs" % (name, relu, int((_bits(p) != _bits(want)).sum()))
        if relu == 0 or _family(name) == "direct":
            assert np.isnan(y).any() and (want == -np.inf).any(), "%s: no all-NaN window was produced" % name
        only = run(name, x, w, b, relu, POOLED)[1].interior()
        assert np.array_equal(_bits(only), _bits(p)), "%s (relu %d): pooled-only launch differs from the tap-layer launch" % (name, relu)


@pytest.mark.parametrize("name", ["pool_c9_7x9", "pool_c200_17x33", "pool_c3_1x5"])
def test_edge_pool_rule_standalone(dev, name):
    c = CASES[name]
    x, _, _ = acc_operands(name, "mixed", 3)
    x[:, :min(3, c["H"]), :3] = np.nan
    x[-1, -1, -1] = np.nan
    x[0, 0, -1] = np.inf
    x[0, -1, 0] = -np.inf
    p = run(name, x)[1].interior()
    want = pool_ref(x)
    assert (want == -np.inf).any() and not np.isnan(p).any()
    assert np.array_equal(_bits(p), _bits(want))


# ---------------------------------------------------------------------------------------------------------------------------------------
# tier 4: invariance
# ---------------------------------------------------------------------------------------------------------------------------------------
def _words(r):
    return tuple(None if a is None else a.w.copy() for a in r)


def _same(a, b):
    return all((p is None and q is None) or np.array_equal(p, q) for p, q in zip(a, b))


INV = ["d1_c24_4x32_o7", "d2_c9_7x17_o63", "d5_c24_7x31_o129", "d1_s3_c100_9x17_o7", "d2_s3_c96_9x17_o65", "d3_s8_c128_7x31_o200",
       "d4_s2_c96_17x33_o63", "d5_s3_c96_9x15_o129", "d6_s8_c128_17x16_o7", "w8_c24_17x33_o65", "w8_s2_c96_17x33_o65", "w8_s8_c128_15x16_o7",
       "w8_t2_c24_40x40_o65", "w8_t3_c96_57x31_o64", "w16_c512_17x33_o64", "w16_s3_c100_9x31_o128", "w16_s4_c512_17x33_o64",
       "w16_t2_c24_23x65_o129", "w16_t8_c128_31x33_o8", "wbi_c64_7x7_o72", "first_c3_17x33_o72", "pool_c200_17x33"]
STALE_BIG = ("d3_s8_c128_7x31_o200", "w8_t3_c96_57x31_o64")   # larger split layers: they leave the split-K scratch full of their slabs
STALE_SMALL = "d2_c8_9x31_o65"                                 # a small unsplit layer


@pytest.mark.parametrize("name", INV)
def test_repeatable_and_history_blind(dev, name):
    """bit-identical (raw buffers, halo included) run to run, after larger split layers left stale slabs in the split-K scratch, and after a
    small unsplit layer"""
    c = CASES[name]
    x, w, b = acc_operands(name, "wide", 21)
    mode = BOTH if BOTH in c["modes"] else c["modes"][0]
    base = _words(run(name, x, w, b, 1, mode))
    assert _same(base, _words(run(name, x, w, b, 1, mode))), "%s: two runs differ" % name
    for big in STALE_BIG:
        xb, wb, bb = acc_operands(big, "wide", 5)
        run(big, xb * 1.0e3, wb, bb, 0, FULL)
        assert _same(base, _words(run(name, x, w, b, 1, mode))), "%s: result depends on what %s left behind" % (name, big)
    xs, ws, bs = acc_operands(STALE_SMALL, "mixed", 5)
    run(STALE_SMALL, xs, ws, bs, 1, FULL)
    assert _same(base, _words(run(name, x, w, b, 1, mode))), "%s: result differs after a small unsplit layer" % name


def _wino_term_bound(x, w):
    """T[co, y, x] = sum over cin of (sum over taps |w|) x (sum of |x| over the 4x4 input patch of the output's 2x2 tile): bounds every term
    |U_k V_k| of every Winograd component's channel sum (|G| entries <= 1, B^T d B sums 4 of the 16 patch values)"""
    Cin, H, W = x.shape
    th, tw = (H + 1) // 2, (W + 1) // 2
    xp = np.zeros((Cin, 2 * th + 2, 2 * tw + 2))
    xp[:, 1:H + 1, 1:W + 1] = np.abs(x.astype(np.float64))
    P = torch.nn.functional.avg_pool2d(torch.from_numpy(xp)[None], 4, stride=2)[0].numpy() * 16.0    # [Cin, th, tw]
    S = np.abs(w.astype(np.float64)).sum(axis=(2, 3))                                                 # [Cout, Cin]
    T = np.einsum("oc,cyx->oyx", S, P)
    return np.repeat(np.repeat(T, 2, axis=1), 2, axis=2)[:, :H, :W]


@pytest.mark.parametrize("name", SPLITS)
def test_split_matches_unsplit(dev, name):
    """split-K and tail split against the unsplit launch of the same kernel: bit-equal on the exact tier's operands (full and pooled map);
    on random operands within fp32 reassociation of the channel sum — direct: both are sums of the same K = 9 Cin8 products (+ bias) in
    another grouping, |ys - yu| <= 2 (K + 1) 2^-24 (sum |x w| + |b|); Winograd: the transforms are the same per chunk, each of the 9
    components of an output re-groups a Cin8-term sum whose terms _wino_term_bound bounds, |ys - yu| <= 2 x 9 (Cin8 + 9) 2^-24 T"""
    c = CASES[name]
    nch = (c["Cin"] + 7) // 8
    unsplit = dict(knobs=dict(conv_split=1), plan=c["plan"][:2] + (1, nch, 0, 0, 0, 0))
    x, w, b = exact_operands(name, 1)
    for relu in (0, 1):
        assert _same(_words(run(name, x, w, b, relu, BOTH)), _words(run(name, x, w, b, relu, BOTH, **unsplit))), "%s: split differs on exact operands" % name
    x, w, b = acc_operands(name, "mixed", 33)
    ys = run(name, x, w, b, 0, FULL)[0].interior().astype(np.float64)
    yu = run(name, x, w, b, 0, FULL, **unsplit)[0].interior().astype(np.float64)
    if _family(name) == "direct":
        tol = 2 * (9 * nch * 8 + 1) * 2.0 ** -24 * ref64(x, w, b, absolute=True)
    else:
        tol = 18 * (nch * 8 + 9) * 2.0 ** -24 * (_wino_term_bound(x, w) + np.abs(b.astype(np.float64))[:, None, None])
    assert (np.abs(ys - yu) <= tol).all(), "%s: split and unsplit differ by %g x the reassociation bound" % (name, (np.abs(ys - yu) / tol).max())


@pytest.mark.parametrize("name", CONVS)
def test_fused_pool_equals_standalone(dev, name):
    """the fused ceil-mode pool (pooled-only and tap-layer launches) equals maxpool2x2_c8p of the same form's full map, bit for bit"""
    c = CASES[name]
    x, w, b = acc_operands(name, "mixed", 41)
    for relu in (1, 0):
        full, pooled = run(name, x, w, b, relu, BOTH)
        y = full.interior()
        assert np.array_equal(_bits(y), _bits(run(name, x, w, b, relu, FULL)[0].interior())), "%s: the tap-layer launch's full map differs" % name
        Cout, H, W = y.shape
        alone = run("pool_c9_7x9", y, plan=(-1, 0, 0, 0, 0, 0, 0, 0))[1]
        assert alone.outside_untouched() == 0
        assert np.array_equal(_bits(pooled.interior()), _bits(alone.interior())), "%s (relu %d): fused pool != maxpool2x2_c8p of the full map" % (name, relu)
        assert np.array_equal(_bits(run(name, x, w, b, relu, POOLED)[1].interior()), _bits(alone.interior()))


@pytest.mark.parametrize("name", ["wbi_c64_7x7_o72", "wbi_c24_41x15_o8", "wbi_c512_41x33_o64"])
def test_batch_invariant_canvas(dev, name):
    """batch_invariant: a map gets the same bits at any (even: the 2x2 tile phase) height of a taller canvas of zeros, whatever the canvas
    height — the property resnet.hip's per-ROI mosaic relies on.  The plan stays (7, 16, unsplit) whatever the knobs ask for; without
    batch_invariant the same knobs do run a tail split on the tallest canvas"""
    c = CASES[name]
    Cin, H, W, Cout = c["Cin"], c["H"], c["W"], c["Cout"]
    nch = (Cin + 7) // 8
    x, w, b = acc_operands(name, "wide", 9)
    plan = (7, 16, 1, nch, 0, 0, 0, 0)
    base = run(name, x, w, b, 1, FULL)[0].interior()
    assert np.array_equal(_bits(base), _bits(run(name, x, w, b, 1, FULL, knobs=dict(conv_split=-2, wino_tc=8), plan=plan)[0].interior()))
    for Hc, r0 in ((H + 9, 8), (H + 30, 10), (H + 61, 26), (H + 61, 60)):
        canvas = np.zeros((Cin, Hc, W), np.float32)
        canvas[:, r0:r0 + H] = x
        y = run(name, canvas, w, b, 1, FULL, plan=plan)[0].interior()[:, r0:r0 + H]
        # rows next to the map's top / bottom see zeros either way (the canvas is zero around the map, as the halo is)
        assert np.array_equal(_bits(y), _bits(base)), "%s: %d outputs differ at row offset %d of a %d-row canvas" % (name, int((_bits(y) != _bits(base)).sum()), r0, Hc)
    if nch >= 2:
        canvas = np.zeros((Cin, H + 61, W), np.float32)
        canvas[:, 26:26 + H] = x
        run(name, canvas, w, b, 1, FULL, knobs=dict(conv_split=-2), bi=0)
        assert last_plan()[5] >= 2   # the control: without batch_invariant this canvas does split
