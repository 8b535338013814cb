"""tests/tail_cases_np.py on the CPU: every case of tests/test_gpu_tail_boundaries.py can be run by the reference, and does what it is named
for — a threshold ladder whose steps change the reference's own answer, a +-0.0 case in which a -0.0 row precedes a kept +0.0 row, a top-k
table whose first radix pass really has 2049 keys in the bin of the rank.  Without these a case can pass on the GPU for the wrong reason."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tail_cases_np as T  # noqa: E402

F32 = np.float32


@pytest.fixture(scope="module")
def nms_cases(O):
    return T.all_nms_cases(O)


# ------------------------------------------------------------------------------------------------ the reference runs every case
def test_case_sizes_and_names(nms_cases):
    names = [c[0] for c in nms_cases]
    assert len(set(names)) == len(names)
    sizes = {c[1].shape[0] for c in nms_cases}
    assert {3, 5, 64, 65, 130, 257} <= sizes and max(sizes) == 257
    assert set(T.UNDEFINED_IN_NMS_C) <= set(names)


def test_oracle_equals_its_walk_and_nms_c_where_defined(O, nms_cases):
    """O.nms == the step-by-step walk on O.overlap for every (case, threshold); the compiled nms.c agrees bit for bit wherever it is
    defined; the cases in which it reaches `best = -1` are exactly the named list"""
    undefined_seen = set()
    for name, sb, thrs in nms_cases:
        small = sb.shape[0] <= 130
        for thr in thrs:
            keep, idx = O.nms(sb, thr, return_index=True)
            assert T.same_bits(keep, sb[idx]), (name, thr)
            undefined = None
            if small:
                widx, undefined = T.nms_walk(O, sb, thr)
                assert np.array_equal(widx, idx), (name, thr)
            else:  # (the 257-row tables: finite distinct or zero scores, every row pickable)
                undefined = False
                assert name not in T.UNDEFINED_IN_NMS_C and not np.isnan(sb[:, 4]).any() and (sb[:, 4] > T.UNPICK).all()
            if undefined:
                undefined_seen.add(name)
                assert name in T.UNDEFINED_IN_NMS_C, (name, thr)
            elif O.have_ref():
                assert T.same_bits(O.ref_nms(sb, thr), keep), (name, thr)
    assert undefined_seen == set(T.UNDEFINED_IN_NMS_C)


def test_overlap_oracle_equals_nms_c_on_all_case_boxes(O, nms_cases):
    if not O.have_ref():
        pytest.skip("needs the reference's compiled nms.c")
    boxes = np.concatenate([c[1][:, :4] for c in nms_cases if c[1].shape[0] <= 65])
    for b in (T.PICKED, (0, 0, np.inf, np.inf), (-T.BIG, -T.BIG, T.BIG, T.BIG), (np.nan, 0, 9, 9), (10, 10, 5, 5)):
        got = O.boxoverlap(boxes, b)
        ref = np.asarray([O.ref_overlap(a, b) for a in boxes], np.float32)
        assert T.same_bits(got, ref), b


# ------------------------------------------------------------------------------------------------ lattice and ladders
def test_lattice_values_are_the_named_fractions(O):
    for box, (p, q) in T.LATTICE:
        v = F32(O.overlap(T.PICKED, box))
        assert v == F32(p) / F32(q), (box, p, q)
        assert F32(O.overlap(box, T.PICKED)) == v
    exact = [F32(p) / F32(q) for _, (p, q) in T.LATTICE if q in (1, 2, 4, 8)]
    assert sorted(float(v) for v in exact) == [0.125, 0.25, 0.5, 1.0]
    big = T.lattice(257)  # a moved tile has the values of the first
    for i in range(8):
        assert F32(O.overlap(big[248, :4], big[248 + i, :4])) == F32(O.overlap(big[0, :4], big[i, :4]))


def test_every_nms_ladder_value_discriminates(O):
    for builder, at_least in ((T.nms_ladder_lattice, 4), (T.nms_ladder_random, 6)):
        sb, vals = builder(O)
        assert len(vals) >= at_least and len(set(vals)) == len(vals)
        for v in vals:
            at_v = O.nms(sb, float(v), return_index=True)[1]
            below = O.nms(sb, float(T.pred(v)), return_index=True)[1]
            assert not np.array_equal(at_v, below), v     # `iou <= thr` flips for a pair that decides
            assert len(at_v) > len(below) or not np.array_equal(at_v[:len(below)], below), v
    sb, vals = T.nms_ladder_lattice(O)
    assert {0.5, 0.25, 0.125} <= set(float(v) for v in vals)  # the exact fractions are on the ladder (1 cannot be: nothing is above it)
    assert float(F32(1) / F32(3)) in [float(v) for v in vals]


def test_every_vote_ladder_value_discriminates(O):
    """bbox_vote's test is strict: the row with ov == v votes at pred(v) and not at v.  (At v and at succ(v) it votes in neither, so
    those two results differ only if another pair's value is succ(v); the observable step is pred(v) -> v.)"""
    for builder, at_least in ((T.vote_ladder_lattice, 7), (T.vote_ladder_random, 6)):
        kept, sb, vals = builder(O)
        assert len(vals) >= at_least
        for v in vals:
            at_v, below = T.vote_ref(O, kept, sb, float(v)), T.vote_ref(O, kept, sb, float(T.pred(v)))
            assert not T.same_bits(at_v, below), v
            assert T.same_bits(O.bbox_vote(kept, sb, float(v)), at_v)  # the oracle and nms.c agree, NaN rows included
    kept, sb, vals = T.vote_ladder_lattice(O)
    assert {1.0, 0.5, 0.25, 0.125} <= set(float(v) for v in vals)


def test_vote_cases_hit_their_edges(O):
    cases = {c[0]: c for c in T.vote_cases(O)}
    _, kept, sb, thrs, _ = cases["vote_nobody_votes"]
    r = T.vote_ref(O, kept, sb, thrs[0])
    assert np.isnan(r[0, :4]).all() and not np.isnan(r[1, :4]).any() and T.same_bits(r[:, 4], kept[:, 4])  # a4 == 0: NaN in the reference too
    _, kept, sb, thrs, _ = cases["vote_thr_one"]
    assert np.isnan(T.vote_ref(O, kept, sb, 1.0)[:, :4]).all()
    assert not np.isnan(T.vote_ref(O, kept, sb, float(T.pred(1.0)))[:, :4]).any()
    _, kept, sb, thrs, _ = cases["vote_zero_weights"]
    assert np.isnan(T.vote_ref(O, kept, sb, 0.45)[0, :4]).all() and not np.isnan(T.vote_ref(O, kept, sb, 0.2)[0, :4]).any()
    _, kept, sb, thrs, pows = cases["vote_pow"]
    assert pows == (0.5, 2.0) and (sb[:, 4] == 0).any() and (sb[:, 4] < 0).any()
    assert np.isnan(T.vote_pow_table(sb, 0.5)[:, 4]).sum() == 1 and not np.isnan(T.vote_pow_table(sb, 2.0)[:, 4]).any()
    for _, kept, sb, thrs, pows in T.vote_cases(O):
        for p in pows:
            for thr in thrs:
                assert T.same_bits(O.bbox_vote(kept, T.vote_pow_table(sb, p), thr), T.vote_ref(O, kept, sb, thr, p))


# ------------------------------------------------------------------------------------------------ geometry and scores
def test_geometry_cases_hit_their_edges(O):
    g = T.geometry_cases()
    ov = lambda name, i, j: F32(O.overlap(g[name][i, :4], g[name][j, :4]))
    assert ov("inverted", 0, 1) == 0 and ov("width_zero", 0, 1) == 0 and ov("one_pixel_gap", 0, 1) == 0 and ov("one_pixel_gap", 1, 2) == 0
    assert ov("shared_column", 0, 1) == F32(10) / F32(190)
    assert ov("identical", 0, 1) == 1
    assert ov("huge_and_small", 0, 1) == 0 and np.isfinite(F32(T.BIG) * 2 + 1) and (F32(T.BIG) * 2 + 1) > np.sqrt(F32(T.FLT_MAX))  # the area overflows
    assert np.isnan(ov("huge_pair", 0, 1)) and np.isnan(ov("inf_corners", 0, 2)) and np.isnan(ov("nan_corner", 0, 1))
    for name in ("identical", "identical_tied"):  # identical boxes are kept only from thr = 1 on
        assert len(O.nms(g[name], float(T.pred(1.0)))) == 1 and len(O.nms(g[name], 1.0)) == 5
    for name, sb in g.items():  # thr = -1 keeps only the first pick, +inf everything but NaN pairs
        assert len(O.nms(sb, -1.0)) == 1, name


def test_zero_cases_can_see_a_key_that_splits_the_zeros(O):
    """each +-0 case has a -0.0 row BEFORE a +0.0 row with both kept, in that order: a sort that puts +0.0 first gives another answer"""
    for name, sb in T.zero_cases().items():
        for thr in T.ZERO_THRESHOLDS:
            keep, idx = O.nms(sb, thr, return_index=True)
            neg = [i for i in idx if T.bits(sb[i, 4])[0] == 0x80000000]
            pos = [i for i in idx if T.bits(sb[i, 4])[0] == 0]
            assert neg and pos and min(neg) < max(pos), (name, thr)
            order = list(idx)
            assert any(order.index(a) < order.index(b) for a in neg for b in pos if a < b), (name, thr)
            # the answer a +0-first order would give differs: sort the zeros that way and walk
            split = sb.copy()
            split[T.bits(sb[:, 4]) == 0, 4] = T.DENORM  # +0.0 strictly above -0.0
            assert not np.array_equal(O.nms(split, thr, return_index=True)[1], idx), (name, thr)
    z = T.zero_cases()
    assert np.array_equal(O.nms(z["zeros_disjoint4"], 0.3, return_index=True)[1], [0, 1, 2, 3])
    tied_pairs = lambda s: int((np.sort(np.where(s == 0, 0.0, s))[1:] == np.sort(np.where(s == 0, 0.0, s))[:-1]).sum())
    for name in ("zeros_single_pair5", "zeros_single_pair_overlap8", "zeros_single_pair64", "zeros_single_pair130"):
        s = z[name][:, 4]  # the +-0 pair is the class's ONLY tie: with the zeros split, no tied pair is counted and the tie-free scan runs
        assert tied_pairs(s) == 1 and (T.bits(s) == 0x80000000).sum() == 1 and (T.bits(s) == 0).sum() == 1
        assert np.unique(T.bits(s)).size == s.size
    assert 0 < tied_pairs(z["zeros_few_pairs64"][:, 4]) <= 12   # kFewTies: the replaying scan
    assert tied_pairs(z["zeros_run65"][:, 4]) > 12 and tied_pairs(z["zeros_run130"][:, 4]) > 12  # the tie kernel


def test_score_cases_hit_their_edges(O):
    c = T.score_cases()
    s = c["unpick_boundary"][:, 4]
    assert s[0] == F32(-1e7) and s[1] > s[0] and T.bits(s[1])[0] == T.bits(s[0])[0] - 1  # -1e7f and its neighbour towards 0
    idx = O.nms(c["unpick_boundary"], 1.0, return_index=True)[1]
    assert list(idx) == [3, 1]  # the neighbour is picked, -1e7f itself, -2e7 and the next below -1e7f never
    assert len(O.nms(c["all_unpickable"], 0.3)) == 0 and len(O.nms(c["all_unpickable65"], 0.3)) == 0
    assert len(O.nms(c["nan_everywhere"], 0.3)) == 0 and len(O.nms(c["nan_everywhere130"], 0.3)) == 0
    assert list(O.nms(c["unpickable_first_row"], 0.3, return_index=True)[1]) == [1, 2, 3, 4]
    assert list(O.nms(c["plus_inf_fltmax"], 1.0, return_index=True)[1]) == [1, 3, 0, 4, 5, 2]
    assert 0 not in O.nms(c["nan_row0"], 1.0, return_index=True)[1] and 2 not in O.nms(c["nan_middle"], 1.0, return_index=True)[1]
    d = c["denormals"][:, 4]
    assert (d[[0, 1, 3, 5]] != 0).all() and (np.abs(d[[0, 1, 3, 5]]) < np.finfo(np.float32).tiny).all()


# ------------------------------------------------------------------------------------------------ top-k
def test_topk_restatement_equals_the_oracle(O):
    for case in T.topk_cases():
        thr, n_out, rows = T.topk_ref(case)
        per = [case.keep[c, :n] for c, n in enumerate(case.eff_counts)]
        kept, t = O.keep_top_k(per, case.k)
        assert F32(t) == thr, case.name  # (a zero threshold: equal as a value)
        got = np.concatenate([np.concatenate([b, np.full((b.shape[0], 1), c + 1, np.float32)], 1) for c, b in enumerate(kept)]) if n_out else rows
        assert T.same_bits(got, rows), case.name
        assert not np.isnan(case.flat_scores()).any()
        if case.sorted_rows:
            for c, n in enumerate(case.eff_counts):
                assert (np.diff(case.keep[c, :n, 4]) <= 0).all(), case.name


def test_topk_key_map_is_the_kernels():
    s = np.asarray([-np.inf, -T.FLT_MAX, -1.0, -T.DENORM, -0.0, 0.0, T.DENORM, 0.5, 1.0, T.FLT_MAX, np.inf], np.float32)
    k = T.f2key(s)
    assert list(k) == [0x007FFFFF, 0x00800000, 0x407FFFFF, 0x7FFFFFFE, 0x80000000, 0x80000000, 0x80000001, T.K_HALF, 0xBF800000, 0xFF7FFFFF, 0xFF800000]
    assert (np.diff(k.astype(np.int64)) >= 0).all()
    back = T.key2f(k)
    assert T.same_bits(np.where(s == 0, 0.0, s), back)


def _case(name):
    return next(c for c in T.topk_cases() if c.name == name)


def test_topk_cases_reach_the_limits_they_are_named_for():
    by = {}
    for c in T.topk_cases():
        by.setdefault(c.name.rsplit("_k", 1)[0], []).append(c)
    for name, count, adopt_first in (("cand_skipped_then_adopted", 3000, False), ("cand_bin_2048", 2048, True), ("cand_bin_2049", 2049, False)):
        assert len(by[name]) == 3
        ranks = []
        for c in by[name]:
            p = T.topk_first_pass(c)
            assert p["total"] == 6144 <= T.TOPK_LDS and p["shift"] == 16 and p["bin"] == 0x80
            assert p["bin_count"] == count and not p["bin_all_equal"], c.name
            assert (p["bin_count"] <= T.TOPK_CAND) == adopt_first  # the list is filled after the first pass, or skipped
            ranks.append(p["rank_in_bin"])
            # second pass: the range is the bin (65536 keys wide, shift 8); its bin of the rank holds few keys, more than one value wide
            keys = T.f2key(c.flat_scores()).astype(np.int64)
            lo2 = p["lo"] + (p["bin"] << 16)
            in1 = keys[(keys >= lo2) & (keys <= lo2 + 65535)]
            assert in1.size == count and in1.max() - in1.min() >= 256
            srt = np.sort(in1)[::-1]
            b2 = (srt[p["rank_in_bin"] - 1] - in1.min()) >> 8
            assert 0 < ((in1 - in1.min()) >> 8 == b2).sum() <= T.TOPK_CAND  # adopted in the second pass at the latest
        assert ranks == [1, count // 2, count]  # the first, a middle and the last key of the bin
    for total in (32767, 32768, 32769, 32773):
        cs = by["lds_total%d" % total]
        assert all(T.topk_first_pass(c)["total"] == total for c in cs)
        assert {c.k for c in cs} >= {1, total - 1, total, total + 1}
    p = T.topk_first_pass(by["lds_total32769"][0])
    assert p["kth_index"] == 32768  # the k-th key sits in the one row that is not staged
    c = by["lds_total32773"][0]
    p = T.topk_first_pass(c)
    assert p["kth_index"] == 32770
    thr, n_out, rows = T.topk_ref(c)
    flat_idx = rows[:, 0].astype(np.int64) * c.keep.shape[1] + rows[:, 1].astype(np.int64)
    assert sorted(int(i) for i in flat_idx if i >= T.TOPK_LDS) == [32768, 32770, 32771]  # survivors among the rows not staged, and rows that are not
    for name in ("wide0", "wide1", "mix"):
        for c in by[name]:
            p = T.topk_first_pass(c)
            assert p["width"] >= 1 << 31 and p["shift"] == 24, c.name
    # the wide cases meet the 32-bit wrap of `lo + (1 << shift) - 1`: the select in its earlier form ends on FLT_MAX's key where +inf's is due
    wrong = [c.name for n in ("wide0", "wide1", "mix") for c in by[n] if T.topk_passes_wrapping(c) != T.topk_first_pass(c)["kth_key"]]
    assert "wide0_k1" in wrong and "wide1_k1" in wrong and "wide1_k2" in wrong and any(w.startswith("mix") for w in wrong)
    assert T.key2f(T.topk_passes_wrapping(_case("wide0_k1"))) == T.FLT_MAX and T.topk_ref(_case("wide0_k1"))[0] == np.inf
    others = [c for c in T.topk_cases() if not c.name.startswith(("wide", "mix")) and c.flat_scores().size]
    assert all(T.topk_passes_wrapping(c) == T.topk_first_pass(c)["kth_key"] for c in others)  # (the model is the select everywhere else)
    assert {c.max_out for n, v in by.items() if n.startswith("max_out") and not n.startswith("max_out_alt") for c in v} >= {0, 1, 8, 9, 10, 64, 130, 131}
    assert {c.keep.shape[0] for c in T.topk_cases()} >= {64, 65, T.TOPK_MAX_CLS}
    for name, slots, fallback in (("sorted_slots32768", 32768, False), ("sorted_slots32769", 32769, True)):
        c = by[name][0]
        assert c.keep.shape[0] * min(c.k, c.keep.shape[1]) == slots and (slots > T.TOPK_LDS) == fallback
    for name, n_surv in (("tail_ends_on_step", 68), ("tail_ends_before_step", 67), ("tail_ends_after_step", 69), ("tail_ends_on_second_step", 132),
                         ("tail_ends_on_last_row_step", 132), ("tail_ends_on_last_row", 150), ("tail_ends_inside_prefix", 3), ("tail_ends_on_prefix", 4)):
        c = _case(name)
        thr, n_out, rows = T.topk_ref(c)
        assert thr == 1.0 and c.k == 4 and (rows[:, 5] == 2).sum() == n_surv and (rows[:, 5] == 1).sum() == 6 and (rows[:, 5] == 3).sum() == 0
    c = _case("counts_clamped_k3")
    assert list(c.eff_counts) == [4, 0, 0, 4] and (c.counts > c.keep.shape[1]).any() and (c.counts < 0).any()
    assert T.topk_ref(_case("counts_all_empty"))[:2] == (0.0, 0)
