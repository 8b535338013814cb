"""The minibatch sampler without a GPU: the numpy restatement of the two kernels (tests/sampler_np.py) against
the host code it must agree with (train.attach_proposals), against float64, against a transcription of the reference's crowd branch;
the draw's index map; and the argument refusals of the C ABI, which come back before anything touches a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_np as S  # noqa: E402

# the GPU tests' inputs: every case of S.attach_cases()
CPU_CASES = S.attach_cases()


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


def test_restatement_equals_host_attach_proposals_without_crowds():
    from multipathnet_amd import train
    for (n, g, _) in sorted(set((n, g, 0) for (n, g, c) in CPU_CASES)):
        prop, gt, gl, _ = S.make_case(n, g, 0)
        rec, ref = S.attach(prop, gt, gl), train.attach_proposals(prop, gt, gl)
        assert _bits(rec["boxes"], ref["boxes"]) and _bits(rec["overlap"], ref["overlap"]), (n, g)
        assert (rec["corr"] == ref["correspondance"]).all() and (rec["label"] == ref["label"]).all(), (n, g)


def test_host_attach_proposals_with_crowds_equals_restatement():
    from multipathnet_amd import train
    for (n, g, c) in CPU_CASES:
        if not c:
            continue
        prop, gt, gl, crowds = S.make_case(n, g, c)
        rec, ref = S.attach(prop, gt, gl, crowds), train.attach_proposals(prop, gt, gl, crowd_boxes=crowds)
        assert _bits(rec["overlap"], ref["overlap"]), (n, g, c)
        assert (rec["corr"] == ref["correspondance"]).all() and (rec["label"] == ref["label"]).all(), (n, g, c)
        # the default keeps the crowd-free record
        assert _bits(train.attach_proposals(prop, gt, gl)["overlap"], S.attach(prop, gt, gl)["overlap"])


def test_iou_against_float64():
    """The fp32 IoU against float64 on the same fp32 inputs, in units of u = 2^-24 (half an ulp, the cost of one rounding).  The inputs
    are exact, so w and h carry 2 roundings each (the difference, the + 1) and inter 5; each area likewise 5; aarea + barea 6; the
    union = that - inter has absolute error <= 6u (aarea + barea) + 5u inter + u union <= (12 + 5 + 1) u union, as aarea + barea <=
    2 union and inter <= union (no cancellation can amplify it); the quotient 5 + 18 + 1 = 24u.  The bound is 24u relative — a few ulp,
    which is what "ulp-scale" can mean for nine chained operations; the measured figure is printed."""
    prop, gt, gl, _ = S.make_case(1000, 65, 0)
    boxes = np.concatenate([gt, prop], 0).astype(np.float64)
    worst = 0.0
    for j in range(gt.shape[0]):
        o32, _, _ = S.boxoverlap(np.concatenate([gt, prop], 0), gt[j])
        b = gt[j].astype(np.float64)
        w = np.minimum(boxes[:, 2], b[2]) - np.maximum(boxes[:, 0], b[0]) + 1
        h = np.minimum(boxes[:, 3], b[3]) - np.maximum(boxes[:, 1], b[1]) + 1
        inter = w * h
        o64 = inter / ((boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1) + (b[2] - b[0] + 1) * (b[3] - b[1] + 1) - inter)
        o64[(w < 0) | (h < 0)] = 0
        # a box whose fp32 w lands on the other side of 0 than float64's would differ by a whole value: the inputs have none
        assert ((w < 0) == (S.boxoverlap(np.concatenate([gt, prop], 0), gt[j])[1] < 0)).all()
        err = np.abs(o32.astype(np.float64) - o64) / np.maximum(np.abs(o64), 1e-30)
        worst = max(worst, float(err[o64 != 0].max()) if (o64 != 0).any() else 0.0)
    print("IoU fp32 against float64: worst relative error %.3g = %.2f u" % (worst, worst / 2.0 ** -24))
    assert worst <= 24 * 2.0 ** -24


def test_crowd_mask_matches_the_reference_transcription():
    for (n, g, c) in CPU_CASES:
        if not c:
            continue
        prop, gt, gl, crowds = S.make_case(n, g, c)
        rec = S.attach(prop, gt, gl, crowds)
        mask = S.crowd_mask_reference(rec["boxes"], crowds, g)
        assert ((rec["overlap"] == -1) == mask).all(), (n, g, c)
        assert (rec["overlap"][~mask] == rec["overlap_raw"][~mask]).all()
        assert not mask[:g].any()


def test_inputs_hold_the_required_edge_cases():
    """what the GPU test's inputs must contain, shown on the restatement"""
    prop, gt, gl, crowds = S.make_case(65, 3, 2)
    g = 3
    rec = S.attach(prop, gt, gl, crowds)
    assert (gt[0] == gt[1]).all() and rec["corr"][0] == 1 and rec["corr"][1] == 1, "duplicated GT box: the first index wins"
    assert rec["corr"][g + 0] == 0 and rec["label"][g + 0] == 0 and rec["overlap_raw"][g + 0] == 0, "a box disjoint from every GT"
    o, w, h = S.boxoverlap(prop[1:2], S.G0)
    assert w[0] == 0 and o[0] == 0 and rec["overlap_raw"][g + 1] == 0, "touching: w == 0, overlap 0"
    o, w, h = S.boxoverlap(prop[2:3], S.G0)
    assert w[0] < 0 and h[0] > 0 and o[0] == 0, "negative w"
    r, w, h = S.intersection(prop[3:4], S.CROWD0)
    assert w[0] < 0 and h[0] < 0 and r[0] > np.float32(0.7) and rec["overlap"][g + 3] == -1, "both negative: positive, masked though disjoint"
    assert rec["overlap"][g + 4] == -1 and (prop[4] == S.CROWD0).all(), "a proposal identical to a crowd: masked"
    assert S.intersection(gt[0:1], S.CROWD1)[0][0] == 1 and rec["overlap"][0] == 1, "a GT row inside a crowd: not masked"
    assert rec["corr"][g + 3] == 0 and rec["overlap_raw"][g + 3] == 0
    # label and correspondance stay on a masked row: a jittered copy of G0 lies inside crowd 1
    inside = np.nonzero((rec["overlap"] == -1) & (rec["corr"] > 0))[0]
    assert len(inside) and (rec["label"][inside] == gl[rec["corr"][inside] - 1]).all()
    ex = S.exact_threshold_records()
    assert ex["half"]["overlap"][1] == np.float32(0.5) and ex["tenth"]["overlap"][1] == np.float32(0.1)


def test_sampler_cases_are_never_empty():
    for name, (n, g, c, B, ff, ft, lo, hi) in S.SAMPLE_CASES.items():
        prop, gt, gl, crowds = S.make_case(n, g, c)
        out = S.sample(S.attach(prop, gt, gl, crowds), B, ff, ft, lo, hi, seed=555, draw=1)
        assert out["counts"][0] >= 1 and out["counts"][1] >= 1, name
        assert len(out["labels"]) == out["r_bg"] + out["r_fg"] >= 2, name


def test_index_map_stays_in_range():
    words = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], np.uint64)
    for count in (1, 2, 7, 64, 1000, 2 ** 28):
        idx = S.index_map(words, count)
        assert idx.min() == 0 and idx.max() == count - 1, count
    rnd = S.draw_words(555, 3, 1, 4096)
    assert (S.index_map(rnd, 7) < 7).all()


def test_every_index_is_drawn():
    for s in (0, 1):
        idx = S.index_map(S.draw_words(555, 0, s, 4096), 7)
        assert sorted(set(idx.tolist())) == list(range(7)), s
    # the two sets' streams, two draws and two seeds differ
    a = S.draw_words(555, 0, 0, 64)
    assert (a != S.draw_words(555, 0, 1, 64)).any() and (a != S.draw_words(555, 1, 0, 64)).any() and (a != S.draw_words(556, 0, 0, 64)).any()
    assert (a != S.draw_words(555, 1 << 32, 0, 64)).any(), "the high half of `draw` is counter word 3"
    # disjoint from the dropout masks' counters under the same seed: those have counter word 2 = layer < 2^31
    assert (a != S.D.words(555, 0, 0, 64, 1)[:, 0]).any()


def test_sample_layout_on_the_restatement():
    prop, gt, gl, crowds = S.make_case(1000, 3, 2)
    rec = S.attach(prop, gt, gl, crowds)
    out = S.sample(rec, 128, 0.25, 0.5, 0.1, 0.5, seed=555, draw=9)
    r_bg = out["r_bg"]
    assert (out["labels"][:r_bg] == 0).all() and (out["gt"][:r_bg] == 0).all() and (out["labels"][r_bg:] > 0).all()
    assert (rec["overlap"][out["rows"]] != -1).all() and (rec["overlap"] == -1).any()
    fl = S.sample(rec, 128, 0.25, 0.5, 0.1, 0.5, seed=555, draw=9, flip_width=640)
    assert _bits(fl["rois"], S.flip_boxes(out["rois"], 640)) and _bits(fl["gt"], S.flip_boxes(out["gt"], 640))
    assert (fl["rois"][:, 0] <= fl["rois"][:, 2]).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the C ABI's refusals: MPN_EINVAL from the PRODUCT library, no GPU needed
# ---------------------------------------------------------------------------------------------------------------------------------
def _lib():
    import multipathnet_amd
    lib = multipathnet_amd.load()
    lib.mpn_last_error.restype = C.c_char_p
    return lib


def _cfg(batch_size=128, fg_fraction=0.25, fg=0.5, lo=0.1, hi=0.5):
    from multipathnet_amd import _lib as L
    return L.RoiSamplerCfg(batch_size, fg_fraction, fg, lo, hi)


P = C.c_void_p(0x1000)   # a non-null pointer that is never followed: every case below is refused before any launch


def test_attach_refusals():
    lib = _lib()
    bad = [
        (dict(n=-1), b"n < 0"), (dict(g=-1), b"g < 0"), (dict(n_crowd=-1), b"n_crowd < 0"), (dict(n=0, g=0), b"g + n == 0"),
        (dict(prop=None), b"d_proposals is NULL"), (dict(gt=None), b"d_gt is NULL"), (dict(gl=None), b"d_gt_labels is NULL"),
        (dict(crowds=None), b"d_crowds is NULL"), (dict(out0=None), b"d_boxes"), (dict(out3=None), b"d_label"),
    ]
    for kw, msg in bad:
        a = dict(prop=P, n=5, gt=P, gl=P, g=2, crowds=P, n_crowd=1, out0=P, out1=P, out2=P, out3=P)
        a.update(kw)
        rc = lib.mpn_attach_proposals(a["prop"], a["n"], a["gt"], a["gl"], a["g"], a["crowds"], a["n_crowd"], a["out0"], a["out1"], a["out2"], a["out3"], None)
        assert rc == -1 and msg in lib.mpn_last_error(), (kw, lib.mpn_last_error())
        assert b"mpn_attach_proposals" in lib.mpn_last_error()


def test_sampler_refusals():
    lib = _lib()
    nan, inf = float("nan"), float("inf")
    bad = [
        (_cfg(batch_size=0), b"batch_size"), (_cfg(batch_size=-4), b"batch_size"), (_cfg(fg_fraction=-0.1), b"fg_fraction"),
        (_cfg(fg_fraction=1.5), b"fg_fraction"), (_cfg(fg_fraction=nan), b"fg_fraction"), (_cfg(fg_fraction=inf), b"fg_fraction"),
        (_cfg(fg=nan), b"fg_threshold"), (_cfg(fg=inf), b"fg_threshold"), (_cfg(lo=nan), b"bg_lo"), (_cfg(hi=inf), b"bg_hi"),
        (_cfg(lo=0.6, hi=0.5), b"bg_lo > cfg->bg_hi"),
    ]
    for cfg, msg in bad:
        rc = lib.mpn_sample_rois(P, P, P, P, 10, C.byref(cfg), 1, 2, 0, P, P, P, P, None)
        assert rc == -1 and msg in lib.mpn_last_error(), (msg, lib.mpn_last_error())
    ok = _cfg()
    assert lib.mpn_sample_rois(P, P, P, P, 10, None, 1, 2, 0, P, P, P, P, None) == -1 and b"cfg is NULL" in lib.mpn_last_error()
    assert lib.mpn_sample_rois(P, P, P, P, 0, C.byref(ok), 1, 2, 0, P, P, P, P, None) == -1 and b"m > 0" in lib.mpn_last_error()
    assert lib.mpn_sample_rois(P, P, P, P, 10, C.byref(ok), 1, 2, -3, P, P, P, P, None) == -1 and b"flip_width" in lib.mpn_last_error()
    for i in (0, 1, 2, 3, 9, 10, 11, 12):   # every required pointer
        args = [P, P, P, P, 10, C.byref(ok), 1, 2, 0, P, P, P, P, None]
        args[i] = None
        assert lib.mpn_sample_rois(*args) == -1 and b"invalid argument" in lib.mpn_last_error(), i


@pytest.mark.parametrize("entry", ["mpn_frcnn_train_add_sampled", "mpn_mpnet_train_add_sampled"])
def test_train_add_sampled_refuses_a_null_handle(entry):
    lib = _lib()
    cfg, counts = _cfg(), (C.c_int * 2)()
    rc = getattr(lib, entry)(None, P, 10, 10, P, 5, P, P, 1, None, 0, C.byref(cfg), 1, 2, 0, counts, None)
    assert rc == -1 and b"invalid argument" in lib.mpn_last_error()
