"""tests/boxes_np.py (the float64 restatements and fp32 emulations that tests/test_gpu_box_kernels_numerics.py compares the detection head's
score and box kernels with) against the CPU oracle and tests/augment_np.py, on the GPU tests' own shape lists: a wrong restatement cannot agree
with a wrong kernel.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_np as A  # noqa: E402
import boxes_np as R  # noqa: E402

F32, U = np.float32, R.U


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _rel(got, ref):
    ok = np.abs(ref) >= R.TINY
    return float((np.abs(got.astype(np.float64) - ref)[ok] / np.abs(ref)[ok]).max()) if ok.any() else 0.0


@pytest.mark.parametrize("sigma", R.SOFTMAX_SIGMA)
def test_softmax_restatements(O, sigma):
    """the oracle's serial fp32 chain lies within (C + 4) * 2^-24 of the float64 rule (expf 1 ulp twice, C - 1 sums, the quotient); the fp32
    emulation follows the oracle to the two expf's difference"""
    for C in R.SOFTMAX_C_FREE:
        x = R.logits(np.random.default_rng(C), max(R.SOFTMAX_M), C, sigma)
        ref, orc = R.softmax(x), O.softmax(x)
        assert _rel(orc, ref) <= (C + 4) * U, C
        assert _rel(R.softmax_f32(x), ref) <= (C + 4) * U, C
        assert np.abs(ref.sum(1) - 1).max() < 1e-12
        small = ref < R.TINY
        assert (orc[small] <= 2.0 ** -125).all()
        if sigma < 40:
            assert not small.any()


def test_softmax_edge_rows(O):
    inf, nan = np.inf, np.nan
    for C in (2, 21, 64, 129):
        base = R.logits(np.random.default_rng(C), 1, C, 1.0)[0]
        rows = [np.full(C, 0.75, F32), base.copy(), base.copy(), np.full(C, -inf, F32), base.copy(), base.copy()]
        rows[1][C // 2] = inf
        rows[2][C - 1] = -inf
        rows[4][0] = nan
        rows[5][0], rows[5][1] = 3e38, -3e38
        x = np.stack(rows).astype(F32)
        ref, orc = R.softmax(x), O.softmax(x)
        assert np.array_equal(np.isnan(ref), np.isnan(orc))
        assert np.isnan(ref[1]).all() and np.isnan(ref[3]).all() and np.isnan(ref[4]).all()  # inf - inf, and a NaN, poison the row's sum
        assert ref[2, C - 1] == 0 and orc[2, C - 1] == 0 and np.isfinite(ref[2]).all()
        assert ref[5, 1] == 0 and orc[5, 1] == 0
        if C & (C - 1) == 0:
            assert (orc[0] == F32(1.0 / C)).all() and (ref[0] == 1.0 / C).all()
        ok = ~np.isnan(ref)
        assert np.allclose(orc[ok], ref[ok], rtol=(C + 4) * U, atol=0)


@pytest.mark.parametrize("K", R.SOFTMAX_K)
def test_softmax_mean_restatement(O, K):
    for C in (2, 21, 65, 256):
        x = R.logits(np.random.default_rng(K * 1000 + C), 5, K * C, 5.0).reshape(5, K, C)
        p = np.stack([O.softmax(x[:, k]) for k in range(K)])  # [K, M, C]
        chain = R.mean_over_k_f32(np.transpose(p, (1, 0, 2)))
        assert np.array_equal(_bits(chain), _bits(O.mean_over_k(p)))
        assert _rel(chain, R.softmax_mean(x)) <= (C + 4 + K + 1) * U


def _deltas(rng, N, C, sigma, tier1=False):
    d = (rng.standard_normal((N, 4 * C)) * sigma).astype(F32)
    if tier1:
        d.reshape(N, C, 4)[..., 2:] = 0
    return d


MEAN4, STD4 = (0.0, 0.01, -0.02, 0.03), (0.1, 0.1, 0.2, 0.2)


def test_decode_restatements(O):
    for N in R.DECODE_N:
        for C in R.DECODE_C:
            rng = np.random.default_rng(N * 100 + C)
            b = R.rois(rng, N)
            d = _deltas(rng, N, C, 0.3, tier1=True)
            assert np.array_equal(_bits(R.decode_f32(b, d)), _bits(O.bbox_decode(b, d)))
            assert np.array_equal(_bits(R.norm_f32(d, MEAN4, STD4)), _bits(O.bbox_norm(d, MEAN4, STD4)))
            for sigma in (0.3, 2.0):
                d = _deltas(rng, N, C, sigma)
                for norm in ((None, None), (MEAN4, STD4)):
                    dn = d if norm[0] is None else O.bbox_norm(d, *norm)
                    err = np.abs(O.bbox_decode(b, dn).astype(np.float64) - R.decode(b, d, *norm))
                    assert (err <= R.decode_bound(b, d, *norm)).all(), (N, C, sigma, float((err / R.decode_bound(b, d, *norm)).max()))
                    assert (np.abs(R.decode_f32(b, dn).astype(np.float64) - R.decode(b, d, *norm)) <= R.decode_bound(b, d, *norm)).all()


def test_clamp_restatement(O):
    up, dn = lambda v: np.nextafter(F32(v), F32(np.inf)), lambda v: np.nextafter(F32(v), F32(-np.inf))
    vals = [1, up(1), dn(1), 1000, up(1000), dn(1000), 600, up(600), dn(600), -0.0, 0.0, np.inf, -np.inf, np.nan, 3e38, -3e38, 300.5]
    v = np.array([(a, b) for a in vals for b in vals], F32)
    for n_pairs in (v.shape[0], v.shape[0] - 1):
        x = v[:n_pairs]
        got, orc = R.clamp(x, 1000, 600), O.clamp_boxes(x, 1000, 600)
        assert np.array_equal(_bits(got), _bits(orc))
        assert np.array_equal(np.isnan(got), np.isnan(x))  # the `<` / `>` chain passes a NaN through
        if n_pairs % 2 == 0:
            assert np.array_equal(_bits(A.clamp_boxes(x.reshape(-1, 4), 1000, 600)), _bits(got).reshape(-1, 4))


@pytest.mark.parametrize("M,C", R.MERGE_MC)
def test_merge_restatement(M, C):
    rng = np.random.default_rng(M * C)
    W, H = 1000, 600
    sA, sB = rng.random((M, C), dtype=F32), rng.random((M, C), dtype=F32)
    bA, bB = rng.uniform(-50, 1100, (M, 4 * C)).astype(F32), rng.uniform(-50, 1100, (M, 4 * C)).astype(F32)
    s32, b32 = A.merge(sA, bA, sB, bB, W)
    s64, b64 = R.merge(sA, bA, sB, bB, W)
    assert (np.abs(s32 - s64) <= U * np.abs(s64) * 2).all()
    assert (np.abs(b32 - b64) <= 3 * U * (np.abs(bA) + np.abs(bB) + W + 1)).all()
    _, bc = A.merge(sA, bA, sB, bB, W, H, clamp=True)
    assert np.array_equal(_bits(bc), _bits(R.clamp(b32, W, H)))


@pytest.mark.parametrize("m", R.VOTE_M)
def test_vote_restatements(O, m):
    rng = np.random.default_rng(m)
    sb = R.vote_tables(rng, m)
    keep = O.nms(sb, 0.7)
    assert m < 255 or keep.shape[0] >= max(R.VOTE_N_NMS)
    for n in R.VOTE_N_NMS:
        nb = keep[:n]
        f32 = R.vote_f32(nb, sb, 0.3)
        assert np.array_equal(_bits(f32), _bits(O.bbox_vote(nb, sb, 0.3)))
        if O.have_ref():
            assert np.array_equal(_bits(f32), _bits(O.ref_bbox_vote(nb, sb, 0.3)))
        for p in R.VOTE_POW:
            ref, bound = R.vote(nb, sb, 0.3, p)
            got = R.vote_f32(nb, sb, 0.3, p)
            assert (np.abs(got[:, :4] - ref[:, :4]) <= bound).all(), (m, n, p)
            assert np.array_equal(got[:, 4], nb[:, 4])
    # a kept box whose voters all weigh 0: 0 / 0; a negative score under pow 0.5: NaN weights
    z = sb.copy()
    z[:, 4] = 0
    assert np.isnan(R.vote_f32(keep[:3], z, 0.3)[:, :4]).all() and np.isnan(O.bbox_vote(keep[:3], z, 0.3)[:, :4]).all()
    z = sb.copy()
    z[0, 4] = -0.25
    assert np.isnan(R.pow_scores(z, 0.5)[0, 4]) and R.pow_scores(z, 2.0)[0, 4] == F32(0.0625)


@pytest.mark.parametrize("H,W,H2,W2,C", R.scale_cases())
def test_image_scale_restatements(O, H, W, H2, W2, C):
    im = np.random.default_rng(H * 1009 + W).random((C, H, W), dtype=F32)
    orc = O.image_scale(im, H2, W2)
    assert np.array_equal(_bits(R.image_scale(im, H2, W2, F32)), _bits(orc))
    assert (np.abs(orc - R.image_scale(im, H2, W2)) <= R.image_scale_bound(H, W, H2, W2, 1.0)).all()
    # a constant image whose value is a power of two comes back bit for bit: the weights (1 - sf) + sf round to 1, and the box average's
    # numerator repeats the operations of its count.  (Any other constant picks up the roundings of its products: not a property.)
    for v in (1.0, 0.5, -2.0):
        assert np.array_equal(_bits(O.image_scale(np.full((C, H, W), F32(v)), H2, W2)), _bits(np.full((C, H2, W2), F32(v))))
