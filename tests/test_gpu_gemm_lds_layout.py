"""The LDS layout of gemm_c8_pf_kernel (dense.hip), pinned to the element.

The kernel's operands reach LDS by LDS-DMA with the halves of every row whose bit 3 is set swapped (the bank swizzle), and the fragment reads
undo the swap.  A sum over K hides a mis-routed half or row wherever the operands are symmetric; a selector does not:
  * probe A: x[m, k] = 1 + m K + k (distinct integers below 2^24) against one-hot weights w[n, k] = (k == n % K): y[m, n] is exactly
    x[m, n % K] — every output names the one activation element it read;
  * probe B, the mirror: one-hot activations x[m, k] = (k == m % K) against w[n, k] = 1 + n K + k: y[m, n] is exactly w[n, m % K].
Every other product of a sum is 0, so the result is exact in any summation order and is compared with numpy for equality.

Forms are reached through mpn_debug_linear_form with the knobs gemm_kch / gemm_split / gemm_rsi, as tests/test_gpu_gemm_numerics.py does.
A stage holds 8 * kch k; K is padded to 64, so an un-split kch = 4 launch always runs an even number of stages (n_more odd: it starts in
stage buffer 1); one-stage launches and even n_more come from kch = 8 (K = 64, 192) and from split launches (kch = 4: K = 64, 192 in two).
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
KNOB_DEFAULTS = dict(gemm_kch=0, gemm_split=0, gemm_rsi=1)


@functools.lru_cache(maxsize=None)
def _dbg():
    from multipathnet_amd import _lib
    lib = _lib.load("debug")
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    lib.mpn_debug_linear_form.argtypes = [vp, i, i, vp, vp, i, i, i, i, vp, i, C.POINTER(C.c_int), vp, i, i, i, vp, vp, sz]
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


def run(x, w, knobs=None, ri=0, res=None, scales=None, cuts=(), bin_rows=0):
    """y[M, N] (numpy float32), bias 0, no ReLU.  scales [n_seg, rs_mod]: the per-row-scaled form over the K segments ending at cuts;
    bin_rows > 0: its packed (bin, roi) rows, scattered with a gap of 8 never-written rows between bins and gathered back here."""
    from multipathnet_amd import _lib
    lib = _dbg()
    M, K = x.shape
    N = w.shape[0]
    dev = torch.device("cuda", 0)
    xd, wd = torch.from_numpy(np.ascontiguousarray(x)).to(dev), torch.from_numpy(np.ascontiguousarray(w)).to(dev)
    rd = torch.from_numpy(np.ascontiguousarray(res)).to(dev) if res is not None else None
    form, n_seg, rs_mod, out_Mp, kend, sd = 0, 0, 0, 0, None, None
    if scales is not None:
        form, n_seg, rs_mod = 1, scales.shape[0], scales.shape[1]
        sd = torch.from_numpy(np.ascontiguousarray(scales, dtype=np.float32)).to(dev)
        kend = (C.c_int * 2)(*(list(cuts) + [0, 0])[:2])
        out_Mp = bin_rows + 8 if bin_rows else 0
    rows_out = (M // bin_rows) * out_Mp if bin_rows else M
    y = torch.empty((rows_out, N), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    with _knobs(lib, **(knobs or {})):
        rc = lib.mpn_debug_linear_form(_ptr(xd), M, K, _ptr(wd), None, N, 0, form, ri, _ptr(rd), n_seg, kend, _ptr(sd), rs_mod, bin_rows, out_Mp,
                                       _ptr(y), None, 0)
    if rc != 0:
        raise _lib.MpnError("mpn_debug_linear_form failed (%d): %s" % (rc, lib.mpn_last_error().decode()))
    yh = y.cpu().numpy()
    if bin_rows:
        yh = yh.reshape(M // bin_rows, out_Mp, N)[:, :bin_rows].reshape(M, N)
    return yh


# ---------------------------------------------------------------------------------------------------------------------------------------
# the probes
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _probe(which, M, K, N):
    """(x, w, expected y, the k each output selects [M, N])"""
    m, n, k = np.arange(M)[:, None], np.arange(N)[:, None], np.arange(K)[None, :]
    if which == "A":
        x = (1 + m * K + k).astype(np.float32)
        w = (k == n % K).astype(np.float32)
        sel = np.broadcast_to((np.arange(N) % K)[None, :], (M, N))
        y = x[:, np.arange(N) % K]
    else:
        x = (k == m % K).astype(np.float32)
        w = (1 + n * K + k).astype(np.float32)
        sel = np.broadcast_to((np.arange(M) % K)[:, None], (M, N))
        y = w[:, np.arange(M) % K].T
    assert max(x.max(), w.max()) < 2 ** 24
    return x, w, np.ascontiguousarray(y), sel


def _same(y, want, what):
    bad = np.argwhere(y != want)
    assert bad.size == 0, "%s: %d of %d outputs differ, first at (row, col) %s: got %r, want %r" % (
        what, len(bad), y.size, tuple(bad[0]), float(y[tuple(bad[0])]), float(want[tuple(bad[0])]))


MS = [16, 24, 40, 72, 136]      # rows with bit 3 clear / set, both 32-row groups of a wave, a second row tile; all ragged (pad rows)
NS = [105, 128, 136, 264]
PLAIN = [(4, K) for K in (32, 64, 96, 40)] + [(8, K) for K in (64, 128, 192)]
PLAIN_CASES = [(kch, K, M, N) for kch, K in PLAIN for M in MS for N in NS]


@pytest.mark.parametrize("kch,K,M,N", PLAIN_CASES, ids=["kch%d-K%d-M%d-N%d" % c for c in PLAIN_CASES])
def test_selector_unsplit(dev, kch, K, M, N):
    """one block per tile over all of K: kch = 4 runs 2 or 4 stages (n_more odd), kch = 8 one, two or three (one-stage, odd, even)"""
    for which in "AB":
        x, w, want, _ = _probe(which, M, K, N)
        _same(run(x, w, knobs=dict(gemm_kch=kch, gemm_split=1)), want, "probe %s" % which)


SPLIT_CASES = [(4, 128), (4, 64), (4, 192), (8, 128)]  # stages per piece: 2 (odd n_more), 1 (one-stage), 3 (even n_more), 1


@pytest.mark.parametrize("M,N", [(16, 105), (40, 136), (136, 264)])
@pytest.mark.parametrize("kch,K", SPLIT_CASES, ids=["kch%d-K%d" % c for c in SPLIT_CASES])
def test_selector_split2(dev, kch, K, M, N):
    """gemm_split = 2: two blocks per tile into partial slabs, then the reduce kernel"""
    for which in "AB":
        x, w, want, _ = _probe(which, M, K, N)
        _same(run(x, w, knobs=dict(gemm_kch=kch, gemm_split=2)), want, "probe %s" % which)


@pytest.mark.parametrize("M", [1024, 1000])
def test_selector_fold(dev, M):
    """the folding instantiation: 128 tiles, two canonical segments of four stages (row_invariant, N = 2048, K = 256); M = 1000 leaves 24 pad
    rows = three 8-row records in the last row tile"""
    N, K = 2048, 256
    for which in "AB":
        x, w, want, _ = _probe(which, M, K, N)
        _same(run(x, w, ri=1), want, "probe %s" % which)


RS_CASES = [(n_seg, rsi, packed) for n_seg in (2, 3) for rsi in (1, 0) for packed in (0, 1)]


@pytest.mark.parametrize("n_seg,rsi,packed", RS_CASES, ids=["rs%d-%s-%s" % (n, "rsi" if r else "fold", "packed" if p else "plain") for n, r, p in RS_CASES])
def test_selector_rowscaled(dev, n_seg, rsi, packed):
    """per-row-scaled K segments, in place (RSI) and through the running total (FOLD); scales are powers of two, so the selected element times
    its segment's scale (RSI: times the exact ratios of two scales) stays exact.  Packed: 7 bins of 24 rows, a row tile straddles bins."""
    M, K, N = (7 * 24, 96, 136) if packed else (136, 96, 264)
    bin_rows = 24 if packed else 0
    rs_mod = bin_rows if packed else M
    cuts = [64] if n_seg == 2 else [32, 64]
    rng = np.random.default_rng(n_seg * 4 + rsi * 2 + packed)
    scales = (2.0 ** rng.integers(-1, 2, (n_seg, rs_mod))).astype(np.float32)
    for which in "AB":
        x, w, want, sel = _probe(which, M, K, N)
        seg = np.searchsorted(np.array(cuts), sel, side="right")             # segment of the selected k
        s = scales[seg, (np.arange(M) % rs_mod)[:, None]]
        _same(run(x, w, knobs=dict(gemm_rsi=rsi), scales=scales, cuts=cuts, bin_rows=bin_rows), want * s, "probe %s" % which)


@pytest.mark.parametrize("M,N,K", [(136, 264, 96), (40, 105, 32)])
def test_selector_direct_with_residual(dev, M, N, K):
    """the direct form (un-split, C8 output) with an integer residual: y - res is the selector result exactly"""
    res = (np.arange(M * N, dtype=np.int64).reshape(M, N) % 7 - 3).astype(np.float32)
    for which in "AB":
        x, w, want, _ = _probe(which, M, K, N)
        y = run(x, w, knobs=dict(gemm_kch=4, gemm_split=1), res=res)
        _same(y - res, want, "probe %s" % which)


# ---------------------------------------------------------------------------------------------------------------------------------------
# same bits whichever form runs
# ---------------------------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_forms_agree_bit_for_bit_on_a_ragged_shape(dev):
    """M = 136, N = 264, K = 96, random fp32.  K = 96 is four 32-k stages = ONE canonical segment, so the un-split launch and both
    row-invariant forms are the same k-ordered chain per output: equal bits.  Row invariance: the first 40 rows of the 136-row call are the
    40-row call's.  gemm_split = 2 + reduce sums two half chains (another rounding, no bit contract with the un-split chain): within the
    fp32 summation bound (K + 2) u sum |x w| of float64."""
    M, N, K = 136, 264, 96
    rng = np.random.default_rng(136264)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    unsplit = run(x, w, knobs=dict(gemm_kch=4, gemm_split=1))
    ri1, ri2 = run(x, w, ri=1), run(x, w, ri=2)
    assert np.array_equal(_bits(unsplit), _bits(ri1)) and np.array_equal(_bits(unsplit), _bits(ri2))
    for ri in (1, 2):
        assert np.array_equal(_bits(run(x[:40], w, ri=ri)), _bits(unsplit[:40])), ri
    y64 = x.astype(np.float64) @ w.astype(np.float64).T
    D = np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)).T
    for y in (unsplit, run(x, w, knobs=dict(gemm_kch=4, gemm_split=2))):
        assert (np.abs(y.astype(np.float64) - y64) <= (K + 2) * U * D).all()


def test_fold_and_split_reduce_agree_bit_for_bit(dev):
    """The row-invariant contract on the new layout: N = 2048, K = 256 has two canonical segments of four stages.  1024 rows run ONE folding
    block per tile, 136 rows one block per segment + the reduce kernel, and gemm_split = 2 cuts K at the same stage: the first 136 rows
    carry the same bits in all three."""
    N, K = 2048, 256
    rng = np.random.default_rng(2048256)
    x = rng.standard_normal((1024, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    fold = run(x, w, ri=1)
    split_ri = run(x[:136], w, ri=1)
    split2 = run(x[:136], w, knobs=dict(gemm_kch=4, gemm_split=2))
    assert np.array_equal(_bits(fold[:136]), _bits(split_ri))
    assert np.array_equal(_bits(split_ri), _bits(split2))
