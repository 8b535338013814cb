"""Multi-scale testing without a GPU: the numpy restatement of its rules on hand-derived cases, the argument checks of the two new
C entries (they refuse before touching the device), the regenerated LuaJIT cdef and the Lua binding's use of the setter."""
import ctypes as C
import os
import re

import numpy as np

import multiscale_np as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_area_exactly_224_squared_picks_the_unscaled_level():
    box = np.array([[1, 1, 224, 224]], F32)           # w = h = 224: area 50176, d = 0 at s = 1
    assert M.levels(box, [1.0, 2.0]).tolist() == [0]
    assert M.levels(box, [2.0, 1.0]).tolist() == [1]
    assert M.levels(box, [0.5, 2.0, 1.0, 1.5]).tolist() == [2]
    rois, lv = M.project(box, [2.0, 1.0])
    assert lv.tolist() == [1] and rois.tolist() == [[2.0, 1.0, 1.0, 224.0, 224.0]]


def test_equidistant_levels_keep_the_lower_one():
    # a 1 x 1 box: d_0 = |1 * 1 - 50176| = 50175 and, with s_1 the float after 1 (s_1^2 = 1 + 2^-22), d_1 = fl(50176 - 1 - 2^-22) = 50175:
    # the two differences are equal and the first level wins, whichever of the two scales comes first
    s1 = float(np.nextafter(F32(1), F32(2)))
    box = np.array([[5, 5, 5, 5]], F32)
    area = F32(1)
    assert np.abs(area * F32(s1) * F32(s1) - M.TARGET_AREA) == np.abs(area - M.TARGET_AREA) == F32(50175)
    assert M.levels(box, [1.0, s1]).tolist() == [0]
    assert M.levels(box, [s1, 1.0]).tolist() == [0]
    # a box between two levels: the closer one wins, a tie goes to the earlier
    assert M.levels(np.array([[1, 1, 112, 112]], F32), [1.0, 2.0]).tolist() == [1]   # 112^2 * 4 = 224^2


def test_nan_and_infinite_boxes_go_to_level_zero():
    nan, inf = np.nan, np.inf
    boxes = np.array([[nan, 1, 10, 10], [1, 1, inf, 10], [-inf, -inf, inf, inf], [1, 5, inf, 4], [1, 1, 10, nan]], F32)
    # NaN area (every difference NaN), infinite area (every difference +inf: all equal), inf * 0 = NaN (w = inf, h = 4 - 5 + 1 = 0)
    lv = M.levels(boxes, [0.5, 1.0, 2.0])
    assert lv.tolist() == [0, 0, 0, 0, 0]
    rois, _ = M.project(boxes, [0.5, 1.0, 2.0])
    assert (rois[:, 0] == 1).all()
    assert np.isnan(rois[0, 1]) and rois[1, 3] == np.inf


def test_duplicate_capped_scales():
    # a 600 x 1000 image with max_size 1000: every target from 600 up is capped to s = 1 (round(s * 1000) > 1000)
    sc = M.level_scales(600, 1000, [480, 576, 688, 864, 1200], 1000)
    assert sc[:2] == [0.8, 0.96] and sc[2:] == [1.0, 1.0, 1.0]
    assert M.distinct_levels(sc) == [0, 1, 2]
    assert M.canvas(600, 1000, sc) == (600, 1000)
    rng = np.random.default_rng(3)
    c = rng.uniform(1, 900, (500, 2))
    wh = np.exp(rng.uniform(np.log(4), np.log(900), (500, 2)))
    boxes = np.concatenate([c, c + wh], 1).astype(F32)
    assert M.levels(boxes, sc).max() <= 2          # a later level with an equal scale is never picked
    # max_size 2000: five distinct levels, canvas 1200 x 2000
    sc2 = M.level_scales(600, 1000, [480, 576, 688, 864, 1200], 2000)
    assert len(set(sc2)) == 5 and M.canvas(600, 1000, sc2) == (1200, 2000)


def test_pick_scale_matches_the_library():
    import multipathnet_amd
    lib = multipathnet_amd.load()
    for (H, W, t, m) in [(600, 1000, 600, 1000), (600, 1000, 864, 1000), (375, 500, 1200, 2000), (120, 200, 150, 250), (333, 499, 688, 1000)]:
        assert lib.mpn_pick_scale(H, W, float(t), float(m)) == M.pick_scale(H, W, t, m)


def _lib():
    import multipathnet_amd
    lib = multipathnet_amd.load()
    lib.mpn_last_error.restype = C.c_char_p
    return lib


def test_set_scales_and_projection_refuse_bad_arguments_without_a_device():
    lib = _lib()
    good = (C.c_double * 9)(*([600.0] * 9))
    assert lib.mpn_frcnn_set_scales(None, 9, good) == -1 and b"MPN_MAX_SCALES" in lib.mpn_last_error()
    assert lib.mpn_frcnn_set_scales(None, -1, good) == -1 and b"MPN_MAX_SCALES" in lib.mpn_last_error()
    for bad in (0.0, -600.0, float("nan"), float("inf")):
        t = (C.c_double * 3)(480.0, bad, 600.0)
        assert lib.mpn_frcnn_set_scales(None, 3, t) == -1
        assert b"target 1" in lib.mpn_last_error(), bad
    assert lib.mpn_frcnn_set_scales(None, 2, good) == -1 and b"invalid argument" in lib.mpn_last_error()   # the NULL handle
    assert lib.mpn_project_im_rois_levels(None, 10, 0, good, None, None) == -1 and b"MPN_MAX_SCALES" in lib.mpn_last_error()
    assert lib.mpn_project_im_rois_levels(None, 10, 9, good, None, None) == -1
    t = (C.c_double * 2)(1.0, float("nan"))
    assert lib.mpn_project_im_rois_levels(None, 10, 2, t, None, None) == -1 and b"scale 1" in lib.mpn_last_error()
    assert lib.mpn_project_im_rois_levels(None, 0, 2, good, None, None) == 0        # nothing to project
    assert lib.mpn_project_im_rois_levels(None, 10, 2, good, None, None) == -1      # NULL buffers


def test_cdef_declares_the_new_entries():
    txt = open(os.path.join(ROOT, "multipathnet_amd", "lua", "mpn_cdef.lua")).read()
    assert "int mpn_frcnn_set_scales(mpn_frcnn *p, int n_scales, const double *h_targets);" in txt
    assert "int mpn_project_im_rois_levels(const float *d_boxes, int n, int n_scales, const double *h_scales, float *d_rois, void *stream);" in txt
    assert "static const int MPN_MAX_SCALES = 8;" in txt


def test_lua_binding_sets_the_pyramid_for_a_scale_table():
    src = open(os.path.join(ROOT, "multipathnet_amd", "lua", "mpn.lua")).read()
    body = src[src.index("local function set_pyramid"):]
    body = body[: body.index("\nend") + 4]
    assert re.search(r"type\(opt\.scale\) == 'table' and #opt\.scale > 1", body)
    assert re.search(r"C\.mpn_frcnn_set_scales\(self\.handle, #opt\.scale, t\)", body)
    # every model constructor hands its options to it (the other kinds refuse a pyramid loudly instead of running scale[1] alone)
    assert src.count("\n   set_pyramid(self, opt)\n") == 4
    # and a table never reaches cfg.scale_target whole
    assert "type(opt.scale) == 'table' and opt.scale[1] or opt.scale" in src
