"""Dropout behind fc6 / fc7, the parts that need no GPU: the numpy restatement of the generator and the mask (tests/dropout_np.py)
against Philox4x32-10's known answers, the keep fractions, the threshold, and the float64 step with masks against PyTorch-CPU float64
autograd with the same masks (as tests/test_train_cpu.py does without masks)."""
import numpy as np
import torch

import dropout_np as D
import train_np as T
from test_train_cpu import _batch, _head


def test_philox4x32_10_known_answers():
    """Random123's known-answer vectors for philox4x32-10"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = D.philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64))
        assert got.dtype == np.uint32 and tuple(int(v) for v in got) == want, [hex(int(v)) for v in got]
    # vectorised over a leading axis: the same answers
    got = D.philox4x32_10(np.array([k[0] for k in kat], np.uint64), np.array([k[1] for k in kat], np.uint64))
    assert [tuple(int(v) for v in row) for row in got] == [k[2] for k in kat]


def test_addressing_is_row_column_layer_step_seed():
    """word col & 3 of Philox(counter = (row, col >> 2, layer, step), key = (seed lo, seed hi))"""
    seed, step, layer = (0x299f31d0 << 32) | 0xa4093822, 0x03707344, 0x13198a2e
    w = D.words(seed, step, layer, 5, 11)
    assert w.shape == (5, 11)
    for row, col in ((0, 0), (4, 10), (3, 6), (2, 3)):
        want = D.philox4x32_10(np.array([row, col >> 2, layer, step], np.uint64), np.array([0xa4093822, 0x299f31d0], np.uint64))[col & 3]
        assert w[row, col] == want
    # the step enters through its low 32 bits, a negative seed through its two's complement
    assert (D.words(seed, step + (1 << 32), layer, 5, 11) == w).all()
    assert (D.words(-1, 0, 0, 2, 4)[0] == D.philox4x32_10(np.array([0, 0, 0, 0], np.uint64), np.array([0xffffffff] * 2, np.uint64))).all()
    # row r of a larger batch is row r of a smaller one: the mask of a row does not depend on B
    assert (D.words(seed, step, layer, 9, 11)[:5] == w).all()


def test_keep_fractions_at_rate_half():
    """rate 0.5, seed 555, layers 0 / 1, steps 0 / 1 / 2 over 70 x 4096 elements: every keep fraction within 0.5 +- 0.004
    (one sigma of a fair coin over 286720 draws is 0.0009)"""
    fr = [D.keep_mask(555, step, layer, 70, 4096, 0.5).mean() for layer in (0, 1) for step in (0, 1, 2)]
    print("keep fractions", ["%.4f" % f for f in fr])
    assert len(fr) == 6 and all(abs(f - 0.5) <= 0.004 for f in fr), fr
    masks = [D.keep_mask(555, step, layer, 70, 4096, 0.5) for layer in (0, 1) for step in (0, 1)]
    for i in range(4):   # layers and steps draw different masks (two fair masks agree on about half their elements)
        for j in range(i + 1, 4):
            assert abs((masks[i] == masks[j]).mean() - 0.5) <= 0.004


def test_threshold_and_scale():
    """T = floor(rate * 2^32) in double with rate the fp32 value the C ABI takes; s = 1.0f / (1.0f - rate) in fp32"""
    assert D.threshold(0.5) == 0x80000000 and D.threshold(0.25) == 0x40000000 and D.threshold(0.0) == 0
    assert D.threshold(0.1) == 13421773 * 32 == 429496736    # fp32 0.1 = 13421773 * 2^-27 (the double 0.1 would give 429496729)
    assert D.scale(0.5) == np.float32(2.0) and D.scale(0.5).dtype == np.float32
    assert D.scale(0.25) == np.float32(1.0) / np.float32(0.75) and float(D.scale(0.25)) == 1.3333333730697632
    assert D.keep_mask(1, 0, 0, 3, 8, 0.0).all()    # rate 0: word >= 0 always
    m6, m7 = D.multipliers(555, 0, 4, 16, 0.5)
    assert m6.dtype == np.float32 and set(np.unique(m6)) <= {0.0, 2.0} and (m6 != m7).any()


def test_float64_step_with_masks_equals_torch_float64_autograd():
    rng = np.random.default_rng(43)
    K6, F, C, B = 40, 24, 5, 19
    P = _head(rng, K6, F, C)
    mean, std = [0.01, -0.02, 0.03, 0.0], [0.1, 0.1, 0.2, 0.2]
    for rate in (0.5, 0.25):
        batches = [_batch(rng, B, K6, C, n_bg=6, n_far=4) + D.multipliers(555, step, B, F, rate) for step in range(3)]
        for depth in (0, 1, 2):
            ref = D.Sgd64(P, depth=depth, momentum=0.9, weight_decay=5e-4, bbox_weight=1.3, mean=mean, std=std)
            losses = [ref.step(*b, lr=0.05)[0] for b in batches]
            Pt, lt = D.torch_steps(P, batches, 0.05, depth=depth, momentum=0.9, weight_decay=5e-4, bbox_weight=1.3, mean=mean, std=std, dtype=torch.float64)
            for k in T.TENSORS:
                err = np.abs(ref.P[k] - Pt[k]).max() / max(np.abs(Pt[k]).max(), 1e-300)
                assert err <= 1e-10, (rate, depth, k, err)
                if k not in T.TRAINED[depth]:
                    assert (ref.P[k] == np.asarray(P[k])).all()
            assert np.abs(np.array(losses) - np.array(lt)).max() <= 1e-10 * np.abs(np.array(lt)).max()
    # with every element kept at scale 1 the masked step IS train_np's step
    ones = np.ones((B, F))
    a, b = D.Sgd64(P, depth=2, mean=mean, std=std), T.Sgd64(P, depth=2, mean=mean, std=std)
    la, lb = a.step(*batches[0][:4], ones, ones, lr=0.05)[0], b.step(*batches[0][:4], lr=0.05)[0]
    assert la == lb and all((a.P[k] == b.P[k]).all() for k in T.TENSORS)
