"""Horizontal-flip test-time augmentation without a GPU: the numpy restatement against a line-by-line torch
transcription of utils.lua:151-155, its algebra (where flipBoxes is an involution and where it is not; merging a table with its own
mirror), and the C ABI — the header, both libraries, the generated LuaJIT cdef, the Lua binding and the argument checks."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import torch

import augment_np as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
ENTRIES = {
    "mpn_frcnn_set_augment": "int mpn_frcnn_set_augment(mpn_frcnn *p, int enable);",
    "mpn_image_hflip": "int mpn_image_hflip(const float *d_in, int C, int H, int W, float *d_out, void *stream);",
    "mpn_flip_boxes": "int mpn_flip_boxes(const float *d_boxes, int n, int image_width, float *d_out, void *stream);",
}


def _flipBoxes_lua(boxes, image_width):
    """utils.lua:151-155, line by line, on a torch.FloatTensor (select's dimension and index are 1-based there)"""
    flipped = boxes.clone()                                                       # local flipped = boxes:clone()
    flipped.select(1, 0).copy_(-boxes.select(1, 2) + image_width + 1)             # flipped:select(2,1):copy( - boxes:select(2,3) + image_width + 1 )
    flipped.select(1, 2).copy_(-boxes.select(1, 0) + image_width + 1)             # flipped:select(2,3):copy( - boxes:select(2,1) + image_width + 1 )
    return flipped                                                                # return flipped


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def test_flip_boxes_is_the_lua_function():
    rng = np.random.default_rng(1201)
    for W in (1, 7, 500, 1000, 4096, 1 << 24):
        b = rng.uniform(-50, 1.2 * W + 50, (4000, 4)).astype(F32)
        b[:12] = [[1, 1, W, 9], [W, 2, 1, 3], [0.1, 0, 0.3, 0], [np.nan, 1, 5, 5], [3, 1, np.nan, 5], [np.inf, 1, -np.inf, 5],
                  [-0.0, 1, 0.0, 5], [16777215, 1, 16777216, 2], [1e-30, 1, 1e30, 2], [0.5, 1, 1.5, 2], [W + 0.25, 1, W + 0.75, 2],
                  [-1e7, 1, 1e7, 2]]
        ref = _flipBoxes_lua(torch.from_numpy(b), W).numpy()
        got = A.flip_boxes(b, W)
        assert _same_bits(got, ref), W
        assert _same_bits(got[:, [1, 3]], b[:, [1, 3]])             # y is untouched
    # a [n, 5] table (scored boxes) keeps its fifth column, as the clone does
    t = rng.random((9, 5)).astype(F32)
    assert _same_bits(A.flip_boxes(t, 100), _flipBoxes_lua(torch.from_numpy(t), 100).numpy())


def test_flip_boxes_is_an_involution_on_integer_coordinates_only():
    rng = np.random.default_rng(1202)
    for W in (1, 2, 333, 1000, 1 << 20):
        # integer-valued coordinates (pixel boxes, in or out of the image): every intermediate is an integer below 2^24, so exact
        b = rng.integers(-W, 2 * W + 2, (5000, 4)).astype(F32)
        assert _same_bits(A.flip_boxes(A.flip_boxes(b, W), W), b), W
    # not an involution on other values: with W = 2^24 - 2 the sums land where fp32 holds integers only.  x1 = 1.5 flips (as the new
    # x2) to fl(fl(-1.5 + 16777214) + 1) = fl(16777212 + 1) = 16777213 (the tie 16777212.5 goes to the even neighbour), and flipping
    # that back gives fl(fl(-16777213 + 16777214) + 1) = 2, not 1.5
    W = (1 << 24) - 2
    b = np.array([[1.5, 1, 2.5, 2]], F32)
    once = A.flip_boxes(b, W)
    assert once[0, 2] == F32(16777213) and once[0, 0] == F32(16777213)    # x1' = fl(fl(-2.5 + W) + 1): 16777211.5 -> 16777212 (even), + 1
    twice = A.flip_boxes(once, W)
    assert twice[0].tolist() == [2.0, 1.0, 2.0, 2.0] and not _same_bits(twice, b)
    # nor on everyday sub-pixel values: the two roundings of a flip lose low bits that the flip back cannot restore
    c = rng.uniform(1, 1000, (20000, 4)).astype(F32)
    back = A.flip_boxes(A.flip_boxes(c, 1000), 1000)
    assert not _same_bits(back, c)
    assert np.abs(back - c).max() <= 2 * np.spacing(F32(1001))            # but within the rounding of numbers of the image's size


def test_merging_a_table_with_its_own_mirror_changes_nothing():
    rng = np.random.default_rng(1203)
    n, Cn, W, H = 300, 6, 500, 375
    s = rng.random((n, Cn)).astype(F32)
    b = rng.integers(-20, W + 20, (n, 4 * Cn)).astype(F32)                # integer-valued: the flip is exact both ways
    b[:, 1::2] = rng.uniform(-20, H + 20, (n, 2 * Cn)).astype(F32)       # y: any value — (y + y) * 0.5 == y in binary floating point
    mirror = A.flip_boxes(b.reshape(-1, 4), W).reshape(b.shape)
    ms, mb = A.merge(s, b, s, mirror, W)
    assert _same_bits(ms, s)
    assert _same_bits(mb[:, 1::2], b[:, 1::2])
    assert _same_bits(mb, b)
    # with the clamp: exactly the clamp of the table
    _, mc = A.merge(s, b, s, mirror, W, H, clamp=True)
    exp = b.copy().reshape(-1, 4)
    exp[:, [0, 2]] = np.clip(exp[:, [0, 2]], 1, W)
    exp[:, [1, 3]] = np.clip(exp[:, [1, 3]], 1, H)
    assert _same_bits(mc, exp.reshape(b.shape))
    # sub-pixel x: y columns and scores still unchanged, x within the flip's rounding
    b2 = rng.uniform(1, W, (n, 4 * Cn)).astype(F32)
    ms2, mb2 = A.merge(s, b2, s, A.flip_boxes(b2.reshape(-1, 4), W).reshape(b2.shape), W)
    assert _same_bits(ms2, s) and _same_bits(mb2[:, 1::2], b2[:, 1::2])
    assert np.abs(mb2 - b2).max() <= 2 * np.spacing(F32(W + 1))


def test_loop_pairs_the_merged_tables():
    """rule 6 on a toy detect: pass i + 1 starts from SelectBoxes of the merged pass i, only the first pass is clamped, and
    use_rbox_scores drops the first score table and the last box table"""
    W, H, n = 40, 30, 5
    calls = []

    def half(mirrored, boxes):
        calls.append((mirrored, boxes.copy()))
        k = F32(len(calls))
        dx = np.array([2, 0, 2, 0], F32) * (F32(-1) if mirrored else F32(1))
        return np.full((n, 2), k, F32), np.concatenate([boxes, boxes + dx], 1).astype(F32)

    boxes = np.array([[1, 1, 10, 10], [5, 5, 45, 35], [-3, 2, 8, 9], [20, 20, 30, 25], [39, 1, 40, 30]], F32)
    sel = lambda s, b: b[:, 4:8].copy()
    sc, bb = A.tester_tables(half, sel, boxes, W, H, num_iter=2)
    assert [m for m, _ in calls] == [False, True, False, True]
    assert _same_bits(calls[1][1], A.flip_boxes(boxes, W))
    assert sc.shape == (2 * n, 2) and bb.shape == (2 * n, 8)
    assert sc[:n].tolist() == [[1.5, 1.5]] * n and sc[n:].tolist() == [[3.5, 3.5]] * n
    # the mirrored half moved its boxes by -2 in x in ITS frame = +2 in the upright frame: the merged second block is x + 2 exactly
    first = A.clamp_boxes(np.concatenate([boxes, boxes + np.array([2, 0, 2, 0], F32)], 1), W, H)
    assert _same_bits(bb[:n], first)
    assert _same_bits(calls[2][1], first[:, 4:8])                          # pass 2 starts from the MERGED, clamped pass 1
    assert _same_bits(bb[n:, :4], first[:, 4:8])                           # and is not clamped itself
    assert (bb[n:] > W).any()
    calls.clear()
    sc_r, bb_r = A.tester_tables(half, sel, boxes, W, H, num_iter=2, use_rbox_scores=True)
    assert _same_bits(sc_r, sc[n:]) and _same_bits(bb_r, bb[:n])


def test_header_declares_the_three_entries_and_the_version_stays():
    hdr = open(os.path.join(ROOT, "include", "mpn.h")).read()
    for proto in ENTRIES.values():
        assert proto in hdr, proto
    assert re.search(r"#define\s+MPN_VERSION\s+600\b", hdr)
    assert "augment" not in hdr[hdr.index("typedef struct mpn_frcnn_config"):hdr.index("} mpn_frcnn_config;")]   # a setter, not a config field


def test_both_libraries_export_the_entries():
    for name in ("libmpn_hip.so", "libmpn_hip_dbg.so"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "multipathnet_amd", name)]).decode()
        syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        for e in ENTRIES:
            assert e in syms, (name, e)


def test_cdef_is_current_and_declares_the_entries():
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_lua_cdef.py"), "--check"]) == 0
    txt = open(os.path.join(ROOT, "multipathnet_amd", "lua", "mpn_cdef.lua")).read()
    for proto in ENTRIES.values():
        assert proto in txt, proto


def _lib():
    import multipathnet_amd
    lib = multipathnet_amd.load()
    lib.mpn_last_error.restype = C.c_char_p
    return lib


def test_version_and_argument_checks_without_a_device():
    lib = _lib()
    assert lib.mpn_version() == 600
    assert lib.mpn_frcnn_set_augment(None, 1) == -1 and b"invalid argument" in lib.mpn_last_error()      # the NULL handle
    assert lib.mpn_frcnn_set_augment(None, 0) == -1
    assert lib.mpn_flip_boxes(None, 0, 100, None, None) == 0                                             # nothing to flip
    assert lib.mpn_flip_boxes(None, 10, 100, None, None) == -1                                           # NULL buffers
    assert lib.mpn_flip_boxes(None, -1, 100, None, None) == -1
    assert lib.mpn_flip_boxes(None, 0, 0, None, None) == -1                                              # an image has a width
    assert lib.mpn_image_hflip(None, 3, 10, 10, None, None) == -1 and lib.mpn_last_error()
    buf = (C.c_float * 4)()
    assert lib.mpn_image_hflip(buf, 3, 10, 10, buf, None) == -1                                          # in place is refused
    assert lib.mpn_image_hflip(buf, 3, 0, 10, buf, None) == -1


def test_hosts_pass_the_option_on():
    lua = open(os.path.join(ROOT, "multipathnet_amd", "lua", "mpn.lua")).read()
    assert re.search(r"if opt\.test_augment then check\(C\.mpn_frcnn_set_augment\(self\.handle, 1\)", lua)
    assert lua.count("\n   set_augment(self, opt)\n") == 4                   # FastRCNN, MultiPathNet, ResNet, Graph
    det = open(os.path.join(ROOT, "multipathnet_amd", "detect.py")).read()
    assert 'opt.get("test_augment"' in det
    host = open(os.path.join(ROOT, "examples", "c_host", "frcnn_host.c")).read()
    assert "--augment" in host and "mpn_frcnn_set_augment(net, 1)" in host
    import inspect
    from multipathnet_amd import models, nn, utils
    assert inspect.signature(models.FastRCNN.__init__).parameters["augment"].default is False
    assert callable(models.FastRCNN.set_augment) and callable(utils.flipBoxes) and callable(nn.hflip)
