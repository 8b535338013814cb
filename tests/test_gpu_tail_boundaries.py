"""The detection tail after the head — nms.hip's NMS paths, utils.nms_dense, boxoverlap, the two bbox_vote kernels, boxes.hip's two keep_top_k
kernels — at their decision boundaries, bit for bit against nms.c / the CPU oracle / a plain numpy restatement.

The cases are tests/tail_cases_np.py's; tests/test_tail_cases_cpu.py proves on the CPU that each does what it is named for (a ladder step that
changes the reference's own answer, a -0.0 row ahead of a kept +0.0 row, 2049 keys in the first radix bin of the rank, ...).  Here every NMS
case runs on every dispatch path (the product library's own dispatch; the fused kernel; the launch chain; the sweep, tie and replaying-scan
kernels forced), alone and as one class among ragged neighbours; every output lies between guard zones and is pre-filled with a sentinel (rows
past the count must keep it); every launch runs twice and must give the same bytes.  No tolerance appears in this module: every comparison is
of bits (any NaN equals any NaN: an x86 0/0 is the negative quiet NaN, the GPU's the positive one).

What the module found.
  1. Signed zeros on the launch chain and in utils.nms_dense.  Only the fused kernel gave -0.0f and 0.0f one sort key.  nms_sort_kernel and
     dense_rank_scatter_kernel keyed the raw bits, so a +0.0 row sorted before a -0.0 row.  Where the +-0 pair is the class's ONLY tie no tied
     pair was counted (`bad` = 0) and the class took the tie-free scan: five disjoint boxes scored 0.5, -0, 0.25, +0, -0.5 came back in order
     [0, 2, 3, 1, 4] where nms.c keeps [0, 2, 1, 3, 4].  (With two zeros of one sign those two tie with EACH OTHER, the class goes to a tie
     path, and the tie paths compare floats: the issue's own example -0, +0, -0, +0 was right on the parent commit, and so is every forced
     path.)  On the parent commit test_nms_cases[chain-zeros], test_nms_single_zero_pair_through_the_public_entry and
     test_nms_dense_cases[scan-zeros] / [ranksweep-zeros] fail (the dense forms on every +-0 case: [2, 4, 1, 3] for the issue's example); they
     pass now.  All three kernels build their key with nms_sort_key(): a +-0 pair is a tied pair, is counted, flagged and resolved by the
     array order in the existing tie paths.  The chain is the headline pipeline's path for its 1000-row tables.
  2. keep_top_k with a key range at least 2^31 wide.  Both kernels narrowed the range with `hi = min(hi, lo + (1 << shift) - 1)`; with
     shift = 24 and a bin that starts above 0xff000000 the sum wraps, hi falls below lo, the select ends a pass early and the threshold is the
     bin's first key: scores {-1, FLT_MAX, +inf} at k = 1 answered FLT_MAX and kept two rows (test_keep_top_k_cases[*-wide], [*-mix] fail on
     the parent commit; tests/test_tail_cases_cpu.py shows the same in a numpy model of the select).  topk_bin_hi() compares distances.
  3. include/mpn.h said nothing on k <= 0 or n_cls > 1024 for the two top-k entries: the sentence is added there (MPN_EINVAL, nothing
     launched) and asserted here.
  Everything else met every check: the IoU comparisons at v, pred(v), succ(v); degenerate, overflowing and NaN geometry; scores at -1e7f and
  its neighbour, +-inf, FLT_MAX, denormals, NaN; the vote kernels' strict test and their 0 / 0; top-k's candidate list at 2048 / 2049 keys, the
  LDS stage at 32768 +- 1, max_out at the wave slices, 64 / 65 / 1024 classes, the sorted kernel's fallback and tail walk.

One reading of the issue corrected (tests/tail_cases_np.py, vote_discriminates): for the strict `ov > thr` a row with ov == v votes at pred(v)
and not at v, nor at succ(v).  The vote ladders are therefore filtered on "the reference's result at pred(v) differs from the one at v" — the
step on which `>=` for `>` shows — and not on v against succ(v), which no row with ov == v can tell apart.  nms.c is also DEFINED for a NaN IoU
(`NaN <= thr` is false: the row is dropped), so those cases are compared against the compiled nms.c too; the named list of undefined cases
(tail_cases_np.UNDEFINED_IN_NMS_C) holds the unpickable-row and NaN-score cases only.

Mutations tried on scratch copies of the libraries (MI355X), each with the first test that fails on it:
  nms_mask_kernel: `!(iou < thr)` for `!(iou <= thr)`                          test_nms_cases[chain-lattice]
  nms_fused_kernel's mask: the same, both words                               test_nms_cases[default-lattice]
  dense_suppresses: `inter > overlap * uni` for the division                  test_nms_dense_cases[scan-ladder]
  nms.hip built with -ffp-contract at its default                             test_boxoverlap_cases[255-product]
  nms_fused_kernel's key without the zero canonicalisation                    test_nms_cases[default-zeros]
  `s >= -1e7f` in nms_wave_kernel (both sites)                                test_nms_cases[sweep-scores]
  `s >= -1e7f` in nms_sort_kernel's pickable count                            test_nms_cases[chain-scores]
  `s >= -1e7f` in nms_fused_kernel's pickable bit                             test_nms_cases[default-scores]
  bbox_vote_kernel: `ov >= thr`                                               test_bbox_vote_cases[product]
  bbox_vote_batched_kernel: `ov >= thr`                                       test_bbox_vote_batched_cases[product]
  keep_top_k_kernel reading topk_keys[i] for i >= n_lds (all four sites)      test_keep_top_k_cases[product-lds]
  keep_top_k_sorted_kernel's tail walk stopping at the first 64-row step      test_keep_top_k_cases[product-tail]
  the parent commit's libraries (both fixes undone)                           test_nms_cases[chain-zeros]; [product-wide] for top-k
The contraction mutant is seen by boxoverlap only against boxes of the random table: with integer boxes every product is exact, and next to
a small integer area the fused sum rounds as the unfused one; the six-value random ladder happened to hold no pair that it moves, and the
vote kernels' `a0 += sx1 * ss` shows it as well (test_bbox_vote_cases).  The topk_keys mutant reads at most five words past the
staged keys, inside the kernel's own LDS allocation.
Not run: the candidate compaction without its `key <= hi` test.  It cannot be observed without an out-of-bounds write: the extra keys are those
of the bins above the rank's, every later pass filters the list with `key >= lo && key <= hi` again, so the answer is the same as long as
the list fits; where it does not fit (more than 2052 keys at or above the bin) the mutant writes past the kernel's LDS allocation, which no
test may do on purpose.
The module's wall time on the MI355X is 4.4 s (73 tests).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tail_cases_np as T  # noqa: E402
from conftest import hooks  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = 0x7FA5A5A5  # a NaN as a float, an impossible row index / count as an int
GUARD = 64         # sentinel elements either side of every output
MPN_EINVAL = -1
cf, ci = C.c_float, C.c_int

NMS_PATHS = {
    "default": {},                         # the product library's own dispatch: the fused kernel at these sizes
    "fused": dict(nms_fused=2),            # the same kernel on the debug flavour
    "chain": dict(nms_fused=0),            # sort -> mask -> tie / scan -> sweep, the chain's own choice per class
    "sweep": dict(nms_force_exact=1),      # nms_wave_kernel for every class
    "tie": dict(nms_force_exact=2),        # nms_tie_kernel wherever it applies
    "replay": dict(nms_force_exact=3),     # nms_scan_kernel with the position replay for every class
}
FAMILIES = {
    "lattice": lambda n: n.startswith("lattice"),
    "ladder": lambda n: n.startswith("ladder"),
    "geometry": lambda n: n.startswith("geo_"),
    "zeros": lambda n: n.startswith("zeros_"),
    "scores": lambda n: not n.startswith(("lattice", "ladder", "geo_", "zeros_")),
}


class Guarded(object):
    """n 4-byte elements of device memory between two guard zones, everything pre-filled with SENT"""

    def __init__(self, n, dev):
        self.n = int(n)
        self.raw = torch.full((2 * GUARD + self.n,), SENT, dtype=torch.int32, device=dev)

    @property
    def ptr(self):
        return C.c_void_p(self.raw.data_ptr() + 4 * GUARD)

    def host(self):
        h = self.raw.cpu().numpy().view(np.uint32)
        assert (h[:GUARD] == SENT).all() and (h[GUARD + self.n:] == SENT).all(), "a guard zone was written"
        return h[GUARD:GUARD + self.n].copy()


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _lib_now():
    from multipathnet_amd import _lib
    return _lib.load()


def _ok(lib, rc):
    assert rc == 0, (rc, lib.mpn_last_error().decode())


def _f(a):
    return np.ascontiguousarray(a).view(np.float32)


# ------------------------------------------------------------------------------------------------ NMS
@pytest.fixture(scope="module")
def nms_cases(O):
    return T.all_nms_cases(O)


@pytest.fixture(scope="module")
def nms_refs(O, nms_cases):
    """(name, thr) -> (kept rows, indices): computed once, never changed"""
    refs = {}
    for name, sb, thrs in nms_cases:
        for thr in thrs:
            refs[(name, thr)] = O.nms(sb, thr, return_index=True)
    return refs


_neighbour_refs = {}


def _neighbour_ref(O, tab, counts, c, thr):
    key = (tab.shape[1], c, thr)
    if key not in _neighbour_refs:
        _neighbour_refs[key] = O.nms(tab[c, :counts[c]], thr, return_index=True)
    return _neighbour_refs[key]


def run_nms(lib, dev, tab, counts, thr):
    """mpn_nms_batched on tab [n_cls, M, 5] -> raw (keep, idx, n_keep) as int32 bit images"""
    n_cls, M, _ = tab.shape
    d_tab = _dev(tab, dev)
    d_counts = _dev(counts, dev) if counts is not None else None
    keep, idx, nk = Guarded(n_cls * M * 5, dev), Guarded(n_cls * M, dev), Guarded(n_cls, dev)
    _ok(lib, lib.mpn_nms_batched(_p(d_tab), _p(d_counts), ci(n_cls), ci(M), cf(thr), keep.ptr, idx.ptr, nk.ptr, None))
    torch.cuda.synchronize()
    return keep.host().reshape(n_cls, M, 5), idx.host().reshape(n_cls, M), nk.host()


def check_nms_class(keep, idx, nk, ref, ridx, what):
    assert nk == ref.shape[0], (what, nk, ref.shape[0], idx[:max(nk, 0)][:16], ridx[:16])
    assert np.array_equal(idx[:nk], ridx), (what, idx[:nk][:16], ridx[:16])
    assert T.same_bits(_f(keep[:nk]), ref), what
    assert (keep[nk:] == SENT).all() and (idx[nk:] == SENT).all(), (what, "rows past the count were written")


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("path", list(NMS_PATHS))
def test_nms_cases(O, dev, nms_cases, nms_refs, path, family):
    with hooks(**NMS_PATHS[path]):
        lib = _lib_now()
        for name, sb, thrs in nms_cases:
            if not FAMILIES[family](name):
                continue
            tab, counts = T.ragged_neighbours(sb)
            for thr in thrs:
                ref, ridx = nms_refs[(name, thr)]
                what = (path, name, thr)
                a = run_nms(lib, dev, sb[None], None, thr)       # alone: mpn_nms's own form (one class, no counts)
                b = run_nms(lib, dev, sb[None], None, thr)
                assert all(np.array_equal(x, y) for x, y in zip(a, b)), (what, "two runs differ")
                check_nms_class(a[0][0], a[1][0], a[2][0], ref, ridx, what)
                a = run_nms(lib, dev, tab, counts, thr)          # as class 1 of three, ragged
                b = run_nms(lib, dev, tab, counts, thr)
                assert all(np.array_equal(x, y) for x, y in zip(a, b)), (what, "two batched runs differ")
                for c in range(3):
                    r, ri = (ref, ridx) if c == 1 else _neighbour_ref(O, tab, counts, c, thr)
                    check_nms_class(a[0][c], a[1][c], a[2][c], r, ri, what + ("class", c))


def test_nms_single_zero_pair_through_the_public_entry(O, dev):
    """one -0.0 and one +0.0 row and no other tie, through utils.nms on each path: nms.c keeps [0, 2, 1, 3, 4]; a key that splits the zeros
    counts no tie, takes the tie-free scan and gives [0, 2, 3, 1, 4]"""
    from multipathnet_amd import utils
    sb = T.zero_cases()["zeros_single_pair5"]
    ref, ridx = O.nms(sb, 0.3, return_index=True)
    assert ridx.tolist() == [0, 2, 1, 3, 4]
    for path, settings in NMS_PATHS.items():
        with hooks(**settings):
            keep, idx = utils.nms_with_index(_dev(sb, dev), 0.3)
            assert idx.cpu().tolist() == [0, 2, 1, 3, 4], path
            assert T.same_bits(keep.cpu().numpy(), ref), path


# ------------------------------------------------------------------------------------------------ utils.nms_dense
@pytest.mark.parametrize("family", ["lattice", "ladder", "geometry", "zeros"])
@pytest.mark.parametrize("sweep", [0, 1], ids=["scan", "ranksweep"])
def test_nms_dense_cases(O, dev, sweep, family):
    """both forms of mpn_nms_dense against the restatement of utils.lua:402-462; equal scores (+-0.0 among them) in ascending index"""
    from multipathnet_amd import utils
    with hooks(nms_dense_sweep=sweep):
        for name, sb, thrs in T.dense_cases(O):
            if not FAMILIES[family](name):
                continue
            d = _dev(sb, dev)
            for thr in thrs:
                ref = O.nms_dense(sb, thr)
                got = utils.nms_dense(d, thr).cpu().numpy()
                again = utils.nms_dense(d, thr).cpu().numpy()
                assert np.array_equal(got, again), (name, thr, "two runs differ")
                assert np.array_equal(got, ref), (name, thr, got[:16], ref[:16])


# ------------------------------------------------------------------------------------------------ boxoverlap
@pytest.mark.parametrize("flavour", ["product", "debug"])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_boxoverlap_cases(O, dev, nms_cases, n, flavour):
    from multipathnet_amd import _lib
    boxes = np.concatenate([c[1][:, :4] for c in nms_cases if not c[0].startswith("lattice") or c[1].shape[0] == 8])
    ext = np.asarray([[0, 0, np.inf, np.inf], [-T.BIG, -T.BIG, T.BIG, T.BIG], [np.nan, 0, 9, 9], [10, 10, 5, 5], [5, 0, 4, 9]], np.float32)
    boxes = np.concatenate([ext, boxes])
    assert boxes.shape[0] >= 257
    # n rows from the front (the extreme boxes) and, for the larger n, the tail of the case list as well
    a = boxes[:n] if n == 1 else np.concatenate([boxes[:n // 2], boxes[-(n - n // 2):]])
    lib = _lib.load("debug" if flavour == "debug" else "product")
    d_a = _dev(a, dev)
    # four boxes of the random table among the `b`: with integer boxes every product in the IoU is exact or meets a sum of far smaller
    # magnitude, and a fused multiply-add changes nothing; against a box of its own kind 3 to 5 of the 64 random boxes give another quotient
    r64 = T.random64()[:, :4]
    for b in (T.PICKED, (5, 5, 14, 14), (0, 0, np.inf, np.inf), (-T.BIG, -T.BIG, T.BIG, T.BIG), (np.nan, 0, 9, 9), (10, 10, 5, 5),
              tuple(r64[0]), tuple(r64[17]), tuple(r64[33]), tuple(r64[50])):
        ref = O.boxoverlap(a, b)
        outs = []
        for _ in range(2):
            out = Guarded(n, dev)
            _ok(lib, lib.mpn_boxoverlap(_p(d_a), ci(n), (cf * 4)(*[float(v) for v in b]), out.ptr, None))
            torch.cuda.synchronize()
            outs.append(out.host())
        assert np.array_equal(outs[0], outs[1])
        assert T.same_bits(_f(outs[0]), ref), (b, n)


# ------------------------------------------------------------------------------------------------ bbox_vote
@pytest.fixture(scope="module")
def vote_cases(O):
    return T.vote_cases(O)


def _vote_neighbours(O, kept, sb):
    """the case as class 1 of three: kept / scored tables [3, M, 5], n_keep, counts"""
    from conftest import case_seed, random_scored_boxes
    M = max(sb.shape[0], kept.shape[0], 70) + 3
    rng = np.random.default_rng(case_seed("distinct", M, salt=11))
    scored_t = np.stack([random_scored_boxes(rng, M, "distinct", span=200.0) for _ in range(3)])
    counts = np.asarray([40, sb.shape[0], M], np.int32)
    scored_t[1, :sb.shape[0]] = sb
    keep_t = np.full((3, M, 5), -3.0, np.float32)
    nk = []
    for c in range(3):
        k = kept if c == 1 else O.nms(scored_t[c, :counts[c]], 0.3)
        keep_t[c, :k.shape[0]] = k
        nk.append(k.shape[0])
    return keep_t, np.asarray(nk, np.int32), scored_t, counts


@pytest.mark.parametrize("flavour", ["product", "debug"])
def test_bbox_vote_cases(O, dev, vote_cases, flavour):
    """mpn_bbox_vote on every vote case at score_pow 1: the strict `ov > thr` at pred(v), v, succ(v); 0 / 0 where nobody (or only zero
    weights) votes — NaN in nms.c too"""
    from multipathnet_amd import _lib
    lib = _lib.load("debug" if flavour == "debug" else "product")
    for name, kept, sb, thrs, pows in vote_cases:
        if 1.0 not in pows:
            continue
        d_k, d_s = _dev(kept, dev), _dev(sb, dev)
        for thr in thrs:
            ref = T.vote_ref(O, kept, sb, thr)
            outs = []
            for _ in range(2):
                res = Guarded(kept.shape[0] * 5, dev)
                _ok(lib, lib.mpn_bbox_vote(_p(d_k), ci(kept.shape[0]), None, _p(d_s), ci(sb.shape[0]), cf(thr), res.ptr, None))
                torch.cuda.synchronize()
                outs.append(res.host())
            assert np.array_equal(outs[0], outs[1]), (name, thr)
            assert T.same_bits(_f(outs[0]).reshape(-1, 5), ref), (name, thr)


@pytest.mark.parametrize("flavour", ["product", "debug"])
def test_bbox_vote_batched_cases(O, dev, vote_cases, flavour):
    """mpn_bbox_vote_batched: the case as one class among ragged neighbours, at its score_pow values (0.5 and 2 meet a zero and a negative
    score: pow(-0.5, 0.5) is NaN and poisons exactly the rows it votes for)"""
    from multipathnet_amd import _lib
    lib = _lib.load("debug" if flavour == "debug" else "product")
    for name, kept, sb, thrs, pows in vote_cases:
        keep_t, nk, scored_t, counts = _vote_neighbours(O, kept, sb)
        n_cls, M, _ = keep_t.shape
        d_k, d_nk, d_s, d_c = _dev(keep_t, dev), _dev(nk, dev), _dev(scored_t, dev), _dev(counts, dev)
        for p in pows:
            for thr in thrs:
                outs = []
                for _ in range(2):
                    res = Guarded(n_cls * M * 5, dev)
                    _ok(lib, lib.mpn_bbox_vote_batched(_p(d_k), _p(d_nk), _p(d_s), _p(d_c), ci(n_cls), ci(M), cf(thr), cf(p), res.ptr, None))
                    torch.cuda.synchronize()
                    outs.append(res.host())
                assert np.array_equal(outs[0], outs[1]), (name, thr, p)
                got = outs[0].reshape(n_cls, M, 5)
                for c in range(n_cls):
                    ref = T.vote_ref(O, keep_t[c, :nk[c]], scored_t[c, :counts[c]], thr, p)
                    assert T.same_bits(_f(got[c, :nk[c]]), ref), (name, thr, p, c)
                    assert (got[c, nk[c]:] == SENT).all(), (name, thr, p, c, "rows past the kept count were written")


# ------------------------------------------------------------------------------------------------ keep_top_k
TOPK_GROUPS = ("cand", "lds", "wide", "mix", "max_out", "ncls", "counts", "ties", "sorted_slots", "tail")


def run_topk(lib, entry, dev, d_keep, d_counts, case, max_out):
    n_cls, M, _ = case.keep.shape
    out, thr, n_out = Guarded(max_out * 6, dev), Guarded(1, dev), Guarded(1, dev)
    _ok(lib, getattr(lib, entry)(_p(d_keep), _p(d_counts), ci(n_cls), ci(M), ci(case.k), thr.ptr, out.ptr, ci(max_out), n_out.ptr, None))
    torch.cuda.synchronize()
    return thr.host(), n_out.host(), out.host().reshape(max_out, 6)


@pytest.mark.parametrize("group", TOPK_GROUPS)
@pytest.mark.parametrize("flavour", ["product", "debug"])
def test_keep_top_k_cases(dev, flavour, group):
    """mpn_keep_top_k on every case, mpn_keep_top_k_sorted on those whose classes are non-increasing: the threshold's bits, the UNTRUNCATED
    count, the rows in class-major order, the sentinel past min(n_out, max_out) rows, and the two entries equal to each other"""
    from multipathnet_amd import _lib
    lib = _lib.load("debug" if flavour == "debug" else "product")
    tables = {}
    for case in T.topk_cases():
        if not case.name.startswith(group):
            continue
        if id(case.keep) not in tables:
            tables[id(case.keep)] = _dev(case.keep, dev)
        d_keep, d_counts = tables[id(case.keep)], _dev(case.counts, dev)
        rthr, rn, rows = T.topk_ref(case)
        max_out = case.max_out if case.max_out is not None else rn + 3
        w = min(rn, max_out)
        got = {}
        for entry in ("mpn_keep_top_k",) + (("mpn_keep_top_k_sorted",) if case.sorted_rows else ()):
            a = run_topk(lib, entry, dev, d_keep, d_counts, case, max_out)
            b = run_topk(lib, entry, dev, d_keep, d_counts, case, max_out)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (case.name, entry, "two runs differ")
            thr, n_out, out = a
            assert thr[0] == T.bits(rthr).ravel()[0], (case.name, entry, _f(thr)[0], rthr)
            assert n_out[0] == rn, (case.name, entry, n_out[0], rn)
            assert np.array_equal(out[:w], T.bits(rows[:w])), (case.name, entry)
            assert (out[w:] == SENT).all(), (case.name, entry, "rows past min(n_out, max_out) were written")
            got[entry] = a
        if len(got) == 2:
            x, y = got["mpn_keep_top_k"], got["mpn_keep_top_k_sorted"]
            assert all(np.array_equal(p, q) for p, q in zip(x, y)), case.name


@pytest.mark.parametrize("flavour", ["product", "debug"])
def test_keep_top_k_rejects_what_the_header_excludes(dev, flavour):
    """include/mpn.h: k >= 1, 0 <= n_cls <= 1024, m_stride >= 0, max_out >= 0 — anything else is MPN_EINVAL and nothing is launched"""
    from multipathnet_amd import _lib
    lib = _lib.load("debug" if flavour == "debug" else "product")
    case = next(c for c in T.topk_cases() if c.name == "ties_k3")
    d_keep, d_counts = _dev(case.keep, dev), _dev(case.counts, dev)
    for entry in ("mpn_keep_top_k", "mpn_keep_top_k_sorted"):
        for bad in T.TOPK_INVALID:
            a = dict(n_cls=case.keep.shape[0], m_stride=case.keep.shape[1], k=case.k, max_out=8)
            a.update(bad)
            out, thr, n_out = Guarded(8 * 6, dev), Guarded(1, dev), Guarded(1, dev)
            rc = getattr(lib, entry)(_p(d_keep), _p(d_counts), ci(a["n_cls"]), ci(a["m_stride"]), ci(a["k"]), thr.ptr, out.ptr, ci(a["max_out"]),
                                     n_out.ptr, None)
            torch.cuda.synchronize()
            assert rc == MPN_EINVAL, (entry, bad, rc)
            assert (out.host() == SENT).all() and thr.host()[0] == SENT and n_out.host()[0] == SENT, (entry, bad)
        # the limits themselves are accepted: n_cls = 0 answers (0, 0)
        out, thr, n_out = Guarded(8 * 6, dev), Guarded(1, dev), Guarded(1, dev)
        _ok(lib, getattr(lib, entry)(None, None, ci(0), ci(4), ci(1), thr.ptr, out.ptr, ci(8), n_out.ptr, None))
        torch.cuda.synchronize()
        assert _f(thr.host())[0] == 0.0 and n_out.host()[0] == 0 and (out.host() == SENT).all(), entry
