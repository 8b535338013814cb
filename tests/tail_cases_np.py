"""Case builders and restatements for the detection tail at its decision boundaries: NMS (nms.c:59-108), box voting (nms.c:110-142),
utils.nms_dense (utils.lua:402-462) and utils.keep_top_k (utils.lua:75-96).  Shared by tests/test_tail_cases_cpu.py, which proves on the CPU
that every case does what it is named for, and tests/test_gpu_tail_boundaries.py, which runs the kernels on them.

Every case is deterministic and small: the decisions under test are per PAIR of boxes (or per key), so tables have 2 .. 257 rows — except the
top-k tables, whose sizes are the kernel's own limits.  Builders that need the oracle take it as `O` (oracle.mpn_oracle): thresholds are the
fp32 values its `overlap` returns, never a value computed here.

NaN scores are left out of the top-k cases on purpose: utils.keep_top_k sorts the scores with torch.sort, whose comparison gives no defined
order with a NaN among them, so there is no answer to compare with (include/mpn.h says the same).  A zero threshold has no defined SIGN either
(-0.0 == 0.0 for the sort); topk_ref returns +0.0, which is what the kernels return."""
import functools

import numpy as np

F32 = np.float32
INF = F32(np.inf)
NAN = F32(np.nan)
FLT_MAX = np.finfo(np.float32).max
DENORM = F32(1e-45)             # the smallest denormal
UNPICK = F32(-10000000.0)       # nms.c:75: a score must be GREATER than this to be picked
THRESHOLDS_EDGE = (0.0, 0.3, 1.0, -1.0, float("inf"))  # geometry cases run against each


def pred(v):
    return np.nextafter(F32(v), -INF)


def succ(v):
    return np.nextafter(F32(v), INF)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    """bit for bit, any NaN equal to any NaN (an x86 0/0 is the negative quiet NaN, the GPU's the positive one)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def scored(boxes, scores):
    return np.concatenate([np.asarray(boxes, np.float32).reshape(-1, 4), np.asarray(scores, np.float32).reshape(-1, 1)], 1)


# ------------------------------------------------------------------------------------------------ restatements
def nms_walk(O, sb, thr):
    """nms.c:59-108 step by step on the oracle's `overlap`: (kept row indices, undefined).  `undefined` = the reference reaches
    `best = -1` with rows left (nms.c:82 then reads boxes[-1]); the oracle and the kernels stop there."""
    sb = np.asarray(sb, np.float32).reshape(-1, 5)
    cur = list(range(sb.shape[0]))
    kept = []
    thr = F32(thr)
    while cur:
        best, best_s = -1, UNPICK
        for i, r in enumerate(cur):
            if sb[r, 4] > best_s:
                best_s, best = sb[r, 4], i
        if best < 0:
            return np.asarray(kept, np.int32), True
        b = cur[best]
        cur[0], cur[best] = cur[best], cur[0]
        cur = cur[1:]
        kept.append(b)
        good = 0
        for i in range(len(cur)):
            if F32(O.overlap(sb[b, :4], sb[cur[i], :4])) <= thr:
                cur[good], cur[i] = cur[i], cur[good]
                good += 1
        cur = cur[:good]
    return np.asarray(kept, np.int32), False


def pair_values(O, a, b=None):
    """the distinct fp32 IoU values of the pairs (a_i, a_j), i < j — or (a_i, b_j) for two tables —, finite and > 0, ascending"""
    a = np.asarray(a, np.float32)[:, :4]
    vals = set()
    if b is None:
        for i in range(len(a)):
            for j in range(i + 1, len(a)):
                vals.add(F32(O.overlap(a[i], a[j])))
    else:
        b = np.asarray(b, np.float32)[:, :4]
        for i in range(len(a)):
            for j in range(len(b)):
                vals.add(F32(O.overlap(a[i], b[j])))
    return sorted(v for v in vals if np.isfinite(v) and v > 0)


def vote_pow_table(sb, score_pow):
    """Tester_FRCNN.lua:119-121: scores:pow(p) on a clone of the scored boxes — THFloatTensor_pow = C pow on the score promoted to double,
    rounded to float once; p == 1 leaves the table as it is"""
    sb = np.array(sb, np.float32)
    if score_pow != 1.0:
        with np.errstate(all="ignore"):
            sb[:, 4] = np.power(sb[:, 4].astype(np.float64), np.float64(F32(score_pow))).astype(np.float32)
    return sb


def vote_ref(O, kept, sb, thr, score_pow=1.0):
    """the reference's own bbox_vote where it is built, else the oracle's"""
    t = vote_pow_table(sb, score_pow)
    return O.ref_bbox_vote(kept, t, thr) if O.have_ref() else O.bbox_vote(kept, t, thr)


# ------------------------------------------------------------------------------------------------ lattice
PICKED = (0, 0, 9, 9)  # 10 x 10 pixels under the +1 convention
# (box, its exact IoU with PICKED as a fraction)
LATTICE = (
    ((0, 0, 9, 9), (1, 1)),
    ((0, 0, 9, 4), (1, 2)),      # 50 / 100
    ((0, 0, 4, 4), (1, 4)),      # 25 / 100
    ((0, 0, 9, 79), (1, 8)),     # 100 / 800
    ((5, 0, 14, 9), (1, 3)),     # 50 / 150   (test.lua:40-52's values: inexact in fp32)
    ((5, 5, 14, 14), (1, 7)),    # 25 / 175
    ((0, 4, 9, 13), (3, 7)),     # 60 / 140
)
LATTICE_SIZES = (8, 65, 130, 257)


def lattice(n=8):
    """n rows: tiles of [PICKED, the seven LATTICE boxes], tile t moved 1000 t pixels to the right (integers far below 2^24: every
    difference stays exact).  Scores are distinct dyadic fractions, PICKED the highest of its tile."""
    rows = []
    tmpl = (PICKED,) + tuple(b for b, _ in LATTICE)
    for i in range(n):
        t, q = divmod(i, 8)
        b = tmpl[q]
        rows.append([b[0] + 1000 * t, b[1], b[2] + 1000 * t, b[3], 1.0 - q / 16.0 - t / 4096.0])
    return np.asarray(rows, np.float32)


def lattice_thresholds():
    out = []
    for _, (p, q) in LATTICE:
        v = F32(p) / F32(q)
        out += [pred(v), v, succ(v)]
    return sorted(set(float(x) for x in out))


# ------------------------------------------------------------------------------------------------ ladders
def nms_discriminates(O, sb, v):
    """the reference's kept set at thr = v differs from the one at pred(v): `iou <= thr` flips for a pair that decides"""
    a, b = O.nms(sb, float(v), return_index=True)[1], O.nms(sb, float(pred(v)), return_index=True)[1]
    return not np.array_equal(a, b)


def vote_discriminates(O, kept, sb, v):
    """`ov > thr` is strict: a row with ov == v votes at pred(v) and not at v (nor at succ(v): the results at v and succ(v) can differ only
    through ANOTHER pair whose value is succ(v)).  The step that shows `>=` for `>` is therefore pred(v) -> v."""
    return not same_bits(O.bbox_vote(kept, sb, float(v)), O.bbox_vote(kept, sb, float(pred(v))))


def ladder(values):
    out = []
    for v in values:
        out += [float(pred(v)), float(v), float(succ(v))]
    return out


@functools.lru_cache(maxsize=None)
def _random64():
    from conftest import case_seed, random_scored_boxes
    return random_scored_boxes(np.random.default_rng(case_seed("distinct", 64, salt=3)), 64, "distinct", span=300.0)


def random64():
    return _random64().copy()


def spread(values, k):
    """k of the values, evenly spaced over the (ascending) list, both ends included"""
    if len(values) <= k:
        return list(values)
    return [values[round(i * (len(values) - 1) / (k - 1))] for i in range(k)]


def nms_ladder_lattice(O):
    sb = lattice(8)
    return sb, [v for v in pair_values(O, sb) if nms_discriminates(O, sb, v)]


def nms_ladder_random(O):
    sb = random64()
    return sb, spread([v for v in pair_values(O, sb) if nms_discriminates(O, sb, v)], 6)


def vote_ladder_lattice(O):
    sb = lattice(8)
    kept = sb[[0]]  # PICKED
    return kept, sb, [v for v in pair_values(O, sb, kept) if vote_discriminates(O, kept, sb, v)]


def vote_ladder_random(O):
    sb = random64()
    kept = O.nms(sb, 0.3)
    return kept, sb, spread([v for v in pair_values(O, sb, kept) if vote_discriminates(O, kept, sb, v)], 6)


# ------------------------------------------------------------------------------------------------ geometry
BIG = 3e19  # (6e19 + 1)^2 overflows fp32: the box's area is +inf


def geometry_cases():
    """name -> [n, 5]; scores distinct and descending unless the case says otherwise.  Each runs against THRESHOLDS_EDGE."""
    g = {}
    g["inverted"] = scored([[0, 0, 20, 20], [10, 10, 5, 5], [12, 12, 3, 18]], [0.9, 0.8, 0.7])          # x2 < x1 (and y2 < y1): negative w, h
    g["width_zero"] = scored([[0, 0, 9, 9], [5, 0, 4, 9], [5, 2, 4, 3]], [0.9, 0.8, 0.7])                # x2 == x1 - 1: w == 0 under +1
    g["shared_column"] = scored([[0, 0, 9, 9], [9, 0, 18, 9], [18, 0, 27, 9]], [0.9, 0.8, 0.7])          # neighbours share ONE pixel column: inter 10
    g["one_pixel_gap"] = scored([[0, 0, 9, 9], [10, 0, 19, 9], [21, 0, 30, 9]], [0.9, 0.8, 0.7])         # w == 0 and w == -1
    g["identical"] = scored([[3, 4, 12, 13]] * 5, [0.9, 0.8, 0.7, 0.6, 0.5])                             # IoU exactly 1: kept only at thr >= 1
    g["identical_tied"] = scored([[3, 4, 12, 13]] * 5, [0.5] * 5)
    g["negative_coords"] = scored([[-20, -20, -11, -11], [-15, -15, -6, -6], [-20, -15, -11, -6], [-1, -1, 0, 0]], [0.9, 0.8, 0.7, 0.6])
    g["huge_and_small"] = scored([[-BIG, -BIG, BIG, BIG], [0, 0, 9, 9], [5, 5, 14, 14]], [0.9, 0.8, 0.7])  # inf area: IoU 100 / inf = 0
    g["small_then_huge"] = scored([[0, 0, 9, 9], [-BIG, -BIG, BIG, BIG], [5, 5, 14, 14]], [0.9, 0.8, 0.7])
    g["huge_pair"] = scored([[-BIG, -BIG, BIG, BIG], [-BIG, -BIG, BIG, BIG], [0, 0, 9, 9]], [0.9, 0.8, 0.7])  # inf / (inf + inf - inf): NaN IoU
    g["inf_corners"] = scored([[0, 0, np.inf, np.inf], [0, 0, 9, 9], [2, 2, np.inf, np.inf]], [0.9, 0.8, 0.7])
    g["inf_corners_low"] = scored([[0, 0, 9, 9], [0, 0, np.inf, np.inf], [-np.inf, -np.inf, 5, 5]], [0.9, 0.8, 0.7])
    g["nan_corner"] = scored([[0, 0, 9, 9], [np.nan, 0, 9, 9], [0, 0, 9, np.nan], [2, 2, 11, 11]], [0.9, 0.8, 0.7, 0.6])
    g["nan_corner_first"] = scored([[np.nan, 0, 9, 9], [0, 0, 9, 9], [2, 2, 11, 11]], [0.9, 0.8, 0.7])
    return g


# ------------------------------------------------------------------------------------------------ scores
def _disjoint(n, step=20):
    return np.asarray([[step * i, 0, step * i + 9, 9] for i in range(n)], np.float32)


def _chain(n, step=5):
    """10 x 10 boxes `step` pixels apart: neighbours overlap (IoU 1/3 at step 5), second neighbours do not"""
    return np.asarray([[step * i, 0, step * i + 9, 9] for i in range(n)], np.float32)


def zero_cases():
    """+-0.0 scores: equal for nms.c:77's '>', so the ARRAY order decides — every case has a -0.0 row before a +0.0 row"""
    z = {}
    z["zeros_disjoint4"] = scored(_disjoint(4), [-0.0, 0.0, -0.0, 0.0])                                  # the issue's own example: kept [0, 1, 2, 3]
    # ONE zero of each sign and no other tie: a key that splits the zeros counts no tied pair at all (two +0.0 rows tie with EACH OTHER, which
    # already sends a class to the tie paths, whose run tests compare floats) — only these reach the tie-free scan with the zeros split
    z["zeros_single_pair5"] = scored(_disjoint(5), [0.5, -0.0, 0.25, 0.0, -0.5])
    z["zeros_single_pair_overlap8"] = scored(_chain(8, step=7), [0.75, 0.5, 0.25, -0.0, 0.0, -0.5, -0.75, -1.0])    # neighbours overlap, IoU 3 / 17
    s = np.linspace(0.9, -0.9, 64).astype(np.float32)
    s[[20, 40]] = [-0.0, 0.0]
    z["zeros_single_pair64"] = scored(_chain(64, step=7), s)
    s = np.linspace(0.9, -0.9, 130).astype(np.float32)
    s[[3, 129]] = [-0.0, 0.0]
    z["zeros_single_pair130"] = scored(_chain(130, step=7), s)
    z["zeros_disjoint_mixed"] =scored(_disjoint(8), [0.5, -0.0, 0.0, -0.25, -0.0, 0.0, 0.75, -1.5])
    z["zeros_overlap"] = scored(_chain(8), [-0.0, 0.0, 0.5, -0.0, 0.0, -0.0, -0.25, 0.0])               # a zero suppresses its neighbour zero
    s = np.linspace(0.9, -0.9, 64).astype(np.float32)
    s[[5, 9, 20, 33, 47, 60]] = [-0.0, 0.0, -0.0, 0.0, 0.0, -0.0]                                        # 5 tied pairs among 64 rows: <= 12, the replaying scan
    z["zeros_few_pairs64"] = scored(_chain(64, step=7), s)
    s = np.linspace(0.9, -0.9, 65).astype(np.float32)
    s[10:50] = np.where(np.arange(40) % 2 == 0, -0.0, 0.0)                                               # 39 tied pairs: > 12, the tie kernel
    z["zeros_run65"] = scored(_chain(65, step=7), s)
    s = np.where(np.arange(130) % 3 == 0, -0.0, 0.0).astype(np.float32)
    s[::10] = np.linspace(0.5, -0.5, 13)
    z["zeros_run130"] = scored(_chain(130, step=6), s)
    s = np.where(np.arange(257) % 2 == 0, -0.0, 0.0).astype(np.float32)                                   # nothing but zeros, more than one 64-rank chunk
    z["zeros_all257"] = scored(_chain(257, step=7), s)
    return z


def score_cases():
    """edge scores; names listed in UNDEFINED_IN_NMS_C reach `best = -1` in nms.c at some threshold"""
    nxt = np.nextafter(UNPICK, F32(0))  # the first pickable score
    c = {}
    c["unpick_boundary"] = scored(_chain(5), [UNPICK, nxt, -2e7, 0.5, np.nextafter(UNPICK, -INF)])
    c["pickable_boundary_only"] = scored(_chain(5), [nxt, nxt, 0.5, nxt, 0.25])                           # all pickable, ties at the boundary
    c["minus_inf"] = scored(_disjoint(5), [0.5, -np.inf, 0.25, -np.inf, 0.1])
    c["plus_inf_fltmax"] = scored(_chain(6), [FLT_MAX, np.inf, -9999999.0, np.inf, FLT_MAX, 1.0])
    c["denormals"] = scored(_chain(8), [DENORM, -DENORM, 0.0, 2 * DENORM, -0.0, DENORM, 1e-38, -1e-38])
    c["unpickable_first_row"] = scored(_disjoint(5), [-2e7, 0.5, 0.4, 0.3, 0.2])
    c["unpickable_first_row_covered"] = scored([[0, 0, 9, 9]] * 3, [-2e7, 0.5, 0.4])                      # suppressed by the pick wherever thr < 1
    c["all_unpickable"] = scored(_disjoint(5), [-2e7, UNPICK, -np.inf, -1e30, -3e7])
    c["all_unpickable65"] = scored(_disjoint(65), np.full(65, UNPICK))
    c["nan_row0"] = scored(_chain(5), [np.nan, 0.5, 0.4, 0.3, 0.2])
    c["nan_middle"] = scored(_chain(5), [0.5, 0.4, np.nan, 0.3, 0.2])
    c["nan_middle65"] = scored(_chain(65, step=7), np.where(np.arange(65) == 32, np.nan, np.linspace(0.9, 0.1, 65)))
    c["nan_everywhere"] = scored(_chain(5), [np.nan] * 5)
    c["nan_everywhere130"] = scored(_chain(130, step=7), np.full(130, np.nan))
    return c


# nms.c:82 reads boxes[-1] when rows are left and none is pickable: a score <= -1e7 or NaN that no pick suppresses.  Checked against the
# oracle only (it stops there, as the kernels do), at the thresholds where it happens.  A NaN IoU is NOT in this class: `NaN <= thr` is
# false, the row is dropped, nms.c is defined and is compared.
UNDEFINED_IN_NMS_C = ("unpick_boundary", "minus_inf", "unpickable_first_row", "unpickable_first_row_covered", "all_unpickable",
                      "all_unpickable65", "nan_row0", "nan_middle", "nan_middle65", "nan_everywhere", "nan_everywhere130")
SCORE_THRESHOLDS = (0.0, 0.3, 1.0)
ZERO_THRESHOLDS = (0.3, 1.0)  # (at 0 the chained boxes suppress their neighbours and too few zeros are left to tell the orders apart)


def all_nms_cases(O):
    """[(name, table, thresholds)] — everything the NMS kernels run"""
    out = [("lattice%d" % n, lattice(n), lattice_thresholds()) for n in LATTICE_SIZES]
    sb, vals = nms_ladder_lattice(O)
    out.append(("ladder_lattice", sb, ladder(vals)))
    sb, vals = nms_ladder_random(O)
    out.append(("ladder_random64", sb, ladder(vals)))
    out += [("geo_" + k, v, THRESHOLDS_EDGE) for k, v in geometry_cases().items()]
    out += [(k, v, ZERO_THRESHOLDS) for k, v in zero_cases().items()]
    out += [(k, v, SCORE_THRESHOLDS) for k, v in score_cases().items()]
    return out


def dense_cases(O):
    """lattice, ladders, geometry and +-0 (finite scores only: utils.nms_dense's sort has no defined place for a NaN)"""
    return [c for c in all_nms_cases(O) if c[0].startswith(("lattice", "ladder", "geo_", "zeros_"))]


def ragged_neighbours(sb, salt=0):
    """the case as class 1 of three: class 0 holds 37 random rows, class 2 a full table; the stride is 3 rows wider than the case"""
    from conftest import case_seed, random_scored_boxes
    n = sb.shape[0]
    M = max(n, 70) + 3
    rng = np.random.default_rng(case_seed("ties", M, salt=salt))
    tab = np.stack([random_scored_boxes(rng, M, r, span=300.0) for r in ("distinct", "ties", "ties")])
    tab[1, :n] = sb
    return tab, np.asarray([37, n, M], np.int32)


# ------------------------------------------------------------------------------------------------ vote
def vote_cases(O):
    """[(name, kept [K,5], scored [m,5], thresholds, score_pows)]"""
    out = []
    kept, sb, vals = vote_ladder_lattice(O)
    out.append(("vote_ladder_lattice", kept, sb, ladder(vals), (1.0,)))
    big = lattice(257)  # more than one 256-row tile of the kernel; kept = every tile's PICKED row: more than one 64-lane block at 33 tiles
    out.append(("vote_lattice257", big[::8], big, lattice_thresholds(), (1.0,)))
    kept, sb, vals = vote_ladder_random(O)
    out.append(("vote_ladder_random64", kept, sb, ladder(vals), (1.0,)))
    lat = lattice(8)
    lonely = scored([[500, 500, 509, 509], [0, 0, 9, 9]], [0.9, 0.8])
    out.append(("vote_nobody_votes", lonely, lat, (0.3,), (1.0,)))                         # a4 == 0: 0 / 0, NaN in the reference too
    out.append(("vote_thr_one", lat[[0, 4]], lat, (1.0, float(pred(1.0))), (1.0,)))       # ov <= 1: nothing votes at 1, the identical row at pred(1)
    zs = lat.copy()
    zs[[0, 1, 2], 4] = [0.0, -0.0, 0.0]
    out.append(("vote_zero_weights", lat[[0, 4]], zs, (0.2, 0.45), (1.0,)))                # at 0.45 only zero-weight rows vote for PICKED: 0 / 0
    ps = lat.copy()
    ps[:, 4] = [0.25, 0.0, -0.5, 4.0, 0.5625, 2.0, 0.75, 1.0]                              # a zero and a negative score: pow(-0.5, 0.5) is NaN
    out.append(("vote_pow", lat[[0, 4, 6]], ps, (0.1, 0.3), (0.5, 2.0)))
    return out


# ------------------------------------------------------------------------------------------------ top-k
TOPK_CAND = 2048     # kTopkCand
TOPK_LDS = 32768     # kTopkLdsKeys
TOPK_MAX_CLS = 1024  # kTopkMaxCls


def f2key(s):
    """the kernels' order-preserving integer image of an fp32 score; -0.0 and +0.0 share a key"""
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, 0, u)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000).astype(np.uint32)


def key2f(k):
    k = np.asarray(k, np.uint64)
    u = np.where(k & 0x80000000, k & 0x7FFFFFFF, ~k & 0xFFFFFFFF).astype(np.uint32)
    return u.view(np.float32)


class TopkCase(object):
    """keep [n_cls, M, 5], counts [n_cls] (as handed to the entry: may exceed M or be negative), k, max_out (None = room for all)"""

    def __init__(self, name, keep, counts, k, max_out=None, sorted_rows=False):
        self.name, self.keep, self.counts, self.k, self.max_out, self.sorted_rows = name, keep, np.asarray(counts, np.int32), int(k), max_out, sorted_rows

    @property
    def eff_counts(self):
        return np.clip(self.counts, 0, self.keep.shape[1])

    def flat_scores(self):
        return np.concatenate([self.keep[c, :n, 4] for c, n in enumerate(self.eff_counts)]) if self.keep.shape[0] else np.zeros(0, np.float32)


def topk_table(per_class_scores, M=None):
    """a table from per-class score lists; the box columns name the row: (class, row, class + row, 7)"""
    n_cls = len(per_class_scores)
    M = M or max(1, max((len(s) for s in per_class_scores), default=1))
    keep = np.full((n_cls, M, 5), -7.0, np.float32)
    keep[:, :, 4] = 0.123  # rows past a class's count: a mid-range score that must never be read
    for c, s in enumerate(per_class_scores):
        s = np.asarray(s, np.float32)
        keep[c, :len(s), 4] = s
        keep[c, :, 0], keep[c, :, 1], keep[c, :, 2] = c, np.arange(M), c + np.arange(M)
    return keep, np.asarray([len(s) for s in per_class_scores], np.int32)


def table_from_flat(scores, n_cls, M):
    """class-major: class c holds flat rows [c M, (c + 1) M); the last class may be short"""
    per = [scores[c * M:(c + 1) * M] for c in range(n_cls)]
    return topk_table(per, M)


def topk_ref(case):
    """utils.lua:75-96 in plain numpy: (thresh, n_out, rows [n_out, 6]) — concatenate class-major, sort descending,
    thresh = s[min(k, total) - 1], survivors `>= thresh` in class-major table order; nothing kept: (0, 0, empty)"""
    flat = case.flat_scores()
    total = flat.size
    if total == 0:
        return F32(0), 0, np.zeros((0, 6), np.float32)
    s = np.sort(flat)[::-1]
    thr = s[min(case.k, total) - 1]
    if thr == 0:
        thr = F32(0.0)  # the sign of a zero threshold is the sort's accident
    rows = []
    for c, n in enumerate(case.eff_counts):
        r = case.keep[c, :n]
        r = r[r[:, 4] >= thr]
        rows.append(np.concatenate([r, np.full((r.shape[0], 1), c + 1, np.float32)], 1))
    rows = np.concatenate(rows)
    return F32(thr), rows.shape[0], rows


def topk_first_pass(case):
    """the kernel's first radix pass in numpy (uint32 arithmetic as the kernel's): lo, hi, width, shift, the bin that holds the rank, its
    population, whether its keys are all equal, and the flat index of the first row that carries the k-th largest key"""
    keys = f2key(case.flat_scores()).astype(np.uint64)
    total = keys.size
    lo, hi = int(keys.min()), int(keys.max())
    width = hi - lo
    nb = width.bit_length()
    shift = nb - 8 if nb > 8 else 0
    hist = np.bincount(((keys - lo) >> shift).astype(np.int64), minlength=256)
    rank = max(min(total, case.k), 1)
    acc, b = 0, 255
    while acc + hist[b] < rank:
        acc += hist[b]
        b -= 1
    in_bin = keys[((keys - lo) >> shift) == b]
    kth = np.sort(keys)[::-1][rank - 1]
    return dict(lo=lo, hi=hi, width=width, shift=shift, bin=b, bin_count=int(hist[b]), bin_all_equal=bool(in_bin.min() == in_bin.max()),
                kth_key=int(kth), kth_index=int(np.flatnonzero(keys == kth)[0]), total=total, rank_in_bin=rank - acc)


def topk_passes_wrapping(case):
    """The radix select with the bin's upper end computed as `min(hi, lo + (1 << shift) - 1)` in 32-bit arithmetic — the form the kernels had
    before this module — : returns the threshold key it ends on.  Differs from the true k-th key when the sum wraps past 2^32."""
    keys = f2key(case.flat_scores()).astype(np.uint64)
    lo, hi = int(keys.min()), int(keys.max())
    rank = max(min(keys.size, case.k), 1)
    while hi > lo:
        nb = (hi - lo).bit_length()
        shift = nb - 8 if nb > 8 else 0
        sel = keys[(keys >= lo) & (keys <= hi)]
        hist = np.bincount(((sel - lo) >> shift).astype(np.int64), minlength=256)
        acc, b = 0, 255
        while acc + hist[b] < rank:
            acc += hist[b]
            b -= 1
        rank -= acc
        lo = (lo + (b << shift)) & 0xFFFFFFFF
        hi = min(hi, (lo + (1 << shift) - 1) & 0xFFFFFFFF)
    return lo


K_HALF = 0xBF000000  # f2key(0.5): keys K_HALF + d, d < 2^24, are the floats in [0.5, 2)


def _keys_to_scores(keys):
    return key2f(np.asarray(keys, np.uint64))


def _three_bins(n_hi, n_mid, n_lo, mid_stride, total):
    """offsets d < 2^24 from K_HALF: d = 0 and 2^24 - 1 pin the range (shift 16, 256 bins of 65536 keys); n_hi keys in bin 0xC0, n_mid in
    bin 0x80 (spread over the bin with `mid_stride`, so that they are not all equal), the rest in bin 0x20.  Shuffled with a fixed seed."""
    assert 2 + n_hi + n_mid + n_lo == total
    d = np.concatenate([[0, 0xFFFFFF], 0xC00000 + (np.arange(n_hi) * 37) % 65536, 0x800000 + (np.arange(n_mid) * mid_stride) % 65536,
                        0x200000 + (np.arange(n_lo) * 11) % 65536]).astype(np.uint64)
    np.random.default_rng(20240517).shuffle(d)
    return _keys_to_scores(K_HALF + d)


@functools.lru_cache(maxsize=None)
def topk_cases():
    cs = []
    # ---- the candidate list (kTopkCand = 2048): the first-pass bin of the rank holds 3000 / 2048 / 2049 keys that are not all equal
    n_cls, M = 3, 2048
    total = n_cls * M
    for name, n_mid in (("cand_skipped_then_adopted", 3000), ("cand_bin_2048", 2048), ("cand_bin_2049", 2049)):
        n_hi = 1500
        s = _three_bins(n_hi, n_mid, total - 2 - n_hi - n_mid, 21, total)
        keep, counts = table_from_flat(s, n_cls, M)
        for k in (1 + n_hi + 1, 1 + n_hi + n_mid // 2, 1 + n_hi + n_mid):  # the first, a middle and the last key of the bin
            cs.append(TopkCase("%s_k%d" % (name, k), keep, counts, k))
    # ---- the LDS stage (kTopkLdsKeys = 32768): totals 32767 / 32768 / 32769 / 32773, threshold and survivors among the rows not staged
    n_cls, M = 17, 2048
    rng = np.random.default_rng(32768)
    base = (K_HALF + rng.permutation(1 << 20)[:TOPK_LDS + 5].astype(np.uint64) * 8 + 8).astype(np.uint64)  # distinct, multiples of 8
    T = int(np.sort(base[:TOPK_LDS])[TOPK_LDS // 2])
    above = int((base[:TOPK_LDS] > T).sum())
    for total in (TOPK_LDS - 1, TOPK_LDS, TOPK_LDS + 1, TOPK_LDS + 5):
        keys = base[:total].copy()
        if total > TOPK_LDS:
            tail = np.asarray([T + 3, T - 5, T + 1, T + 2, T - 1], np.uint64)[:total - TOPK_LDS]  # not staged: the k-th key and survivors
            keys[TOPK_LDS:] = tail
            k_th = above + int((tail > T + 1).sum()) + 1 if total == TOPK_LDS + 5 else above + 1  # T + 1 (index 32770) / T + 3 (index 32768)
        else:
            k_th = above + 1
        keep, counts = table_from_flat(_keys_to_scores(keys), n_cls, M)
        for k in (k_th, 1, total - 1, total, total + 1):
            cs.append(TopkCase("lds_total%d_k%d" % (total, k), keep, counts, k))
    # ---- a key range at least 2^31 wide
    wide = [[-1.0, FLT_MAX, np.inf], [np.inf, 3.0, FLT_MAX, -1.0, np.inf, FLT_MAX]]
    for i, s in enumerate(wide):
        keep, counts = topk_table([s[:len(s) // 2 + 1], s[len(s) // 2 + 1:]])
        for k in range(1, len(s) + 2):
            cs.append(TopkCase("wide%d_k%d" % (i, k), keep, counts, k))
    mix = [[-np.inf, -FLT_MAX, -1.0, -DENORM, -0.0], [0.0, DENORM, 1.0, FLT_MAX, np.inf], [np.inf, -0.0, 0.0, -np.inf, 1e-38, -1e-38, 0.5]]
    keep, counts = topk_table(mix)
    tot = sum(len(s) for s in mix)
    for k in range(1, tot + 2):
        cs.append(TopkCase("mix_k%d" % k, keep, counts, k))
    # ---- max_out: 0, 1 and the wave-slice boundaries of the ordered compaction (16 waves, slices of ceil(total / 16) rows)
    s = np.linspace(2.0, 1.0, 130).astype(np.float32)
    keep, counts = topk_table([s[:60], s[60:61], s[61:]])
    for mo in (0, 1, 8, 9, 10, 17, 18, 19, 63, 64, 65, 129, 130, 131):  # slices of 9 rows; every row survives at k = total
        cs.append(TopkCase("max_out%d" % mo, keep, counts, 130, max_out=mo))
    keep2 = keep.copy()
    keep2[:, :, 4] = np.where(np.arange(keep.shape[1]) % 2 == 0, 2.0, 1.0)  # every other row survives: slices hold 4 or 5 survivors
    for mo in (0, 1, 4, 5, 9, 10, 32, 33):
        cs.append(TopkCase("max_out_alt%d" % mo, keep2, counts, 33, max_out=mo))
    # ---- class counts: 64 / 65 classes (the prefix sum's 64-class steps), kTopkMaxCls; counts above the stride and negative (both clamped)
    for n_cls in (64, 65, TOPK_MAX_CLS):
        rng = np.random.default_rng(n_cls)
        per = [np.round(rng.uniform(-2, 2, int(rng.integers(0, 3))) * 64) / 64 for _ in range(n_cls)]
        per[-1] = np.asarray([1.5, -1.5])  # the last class is never empty
        keep, counts = topk_table(per, M=2)
        tot = int(counts.sum())
        for k in (1, tot // 2, tot - 1, tot, tot + 1):
            cs.append(TopkCase("ncls%d_k%d" % (n_cls, k), keep, counts, k))
    s = [[3.0, 2.5, 2.0, 1.5], [2.75, 2.25, 1.0, 0.5], [9.0, 8.0, 7.0, 6.0], [2.6, 0.1, 0.05, 0.01]]
    keep, counts = topk_table(s)
    for k in (1, 3, 7, 8, 9):
        cs.append(TopkCase("counts_clamped_k%d" % k, keep, [9, -3, 0, 4 + (1 << 20)], k, sorted_rows=True))  # read as [4, 0, 0, 4]
    cs.append(TopkCase("counts_all_empty", keep, [0, -1, 0, -(1 << 30)], 5, sorted_rows=True))
    # ---- k in {1, total - 1, total, total + 1} on a small table of ties
    s = [[1.0, 1.0, 0.5], [1.0, 0.5, 0.5, 0.25], [0.5]]
    keep, counts = topk_table(s)
    for k in (1, 2, 3, 4, 7, 8, 9):
        cs.append(TopkCase("ties_k%d" % k, keep, counts, k, sorted_rows=True))
    # ---- the sorted kernel's fallback: n_cls * min(k, M) = 32768 (its own kernel) / 32769 (the general one); classes non-increasing
    for name, n_cls, M in (("sorted_slots32768", 8, 4096), ("sorted_slots32769", 9, 3641)):
        rng = np.random.default_rng(M)
        per = [np.sort(np.round(rng.uniform(0, 4, int(rng.integers(40, 90))) * 32) / 32)[::-1] for _ in range(n_cls)]
        keep, counts = topk_table(per, M=M)
        tot = int(counts.sum())
        for k in (M, tot, 1 << 20):
            cs.append(TopkCase("%s_k%d" % (name, k), keep, counts, k, sorted_rows=True))
    # ---- the sorted kernel's tail walk: ties at the threshold run past the staged prefix (k rows) and end on a 64-row step, one row to
    # either side, two steps on, or on the class's last row
    k = 4
    for name, plateau, nc in (("ends_on_step", k + 64, 200), ("ends_before_step", k + 63, 200), ("ends_after_step", k + 65, 200),
                              ("ends_on_second_step", k + 128, 200), ("ends_on_last_row_step", k + 128, k + 128), ("ends_on_last_row", 150, 150),
                              ("ends_inside_prefix", 3, 200), ("ends_on_prefix", k, 200)):
        a = np.concatenate([np.full(plateau, 1.0), np.linspace(0.9, 0.1, nc - plateau)]).astype(np.float32)
        b = np.concatenate([[2.0, 1.0, 1.0, 1.0, 1.0, 1.0], np.linspace(0.5, 0.4, 30)]).astype(np.float32)
        keep, counts = topk_table([b, a, [0.5]], M=nc + 3)
        cs.append(TopkCase("tail_" + name, keep, counts, k, sorted_rows=True))
    return tuple(cs)


TOPK_INVALID = (dict(k=0), dict(k=-1), dict(n_cls=TOPK_MAX_CLS + 1), dict(n_cls=-1), dict(max_out=-1), dict(m_stride=-1))  # each answers MPN_EINVAL
