"""COCOeval (bbox) without a GPU: the numpy restatement (tests/cocoeval_np.py) on hand-derived cases, the summary text,
load_coco_gt, and the C ABI's argument checks (mpn_coco_eval_*), which must fail before any device is touched."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cocoeval_np as R  # noqa: E402

P = 1 - 2.0 ** -52   # tp / (tp + fp + eps) of a perfect detector


def _gt(boxes, areas, crowd, ids, img=1, cat=1):
    G = len(ids)
    return {"bbox": np.array(boxes, np.float64).reshape(G, 4), "area": np.array(areas, np.float64),
            "iscrowd": np.array(crowd, np.int64), "image_id": np.full(G, img, np.int64), "category_id": np.full(G, cat, np.int64),
            "id": np.array(ids, np.int64), "img_ids": np.array([img], np.int64), "cat_ids": np.array([cat], np.int64)}


def _rows(dets, img=1, cat=1):
    return np.array([[img] + list(b) + [s, cat] for b, s in dets], np.float32).reshape(-1, 7)


def kat1(gt_id=1):
    return _gt([[0, 0, 20, 20]], [400], [0], [gt_id]), _rows([([0, 0, 20, 10], .9), ([0, 0, 20, 17.5], .8)])


def kat2():
    gt = _gt([[0, 0, 20, 20], [100, 100, 50, 50]], [400, 2500], [0, 1], [1, 2])
    return gt, _rows([([100, 100, 10, 10], .9), ([0, 0, 20, 20], .8), ([110, 110, 10, 10], .7)])


def kat3():
    return _gt([[0, 0, 20, 20]], [400], [0], [0]), _rows([([0, 0, 20, 17.5], .8)])


KATS = {"kat1": kat1, "kat2": kat2, "kat3": kat3}


def test_kat1_threshold_equality_greedy_order_and_maxdets():
    gt, rows = kat1()
    ev = R.evaluate(gt, rows)
    st = R.summarize(ev["precision"], ev["recall"])
    ap = (101 * P + 7 * 101 * 0.5) / 1010
    want = [ap, P, 0.5, ap, -1, -1, 0.1, 0.8, 0.8, 0.8, -1, -1]
    np.testing.assert_allclose(st, want, rtol=0, atol=1e-12)
    assert np.all(ev["precision"][0, :, 0, 0, 2] == P)   # the epsilon quirk: exactly 1 - 2^-52, not 1
    assert np.all(ev["scores"][0, :, 0, 0, 2] == np.float32(.9))


def test_kat2_crowd_iou_reuse_ignored_dets_and_break():
    gt, rows = kat2()
    ev = R.evaluate(gt, rows)
    st = R.summarize(ev["precision"], ev["recall"])
    want = [P, P, P, P, -1, -1, 0, 1, 1, 1, -1, -1]
    np.testing.assert_allclose(st, want, rtol=0, atol=1e-12)


def test_kat3_gt_id_zero_counts_as_false_positive():
    gt, rows = kat3()
    ev = R.evaluate(gt, rows)
    st = R.summarize(ev["precision"], ev["recall"])
    assert st[0] == 0 and st[8] == 0


def test_restatement_refuses_rows_of_unknown_images():
    gt, rows = kat1()
    rows[0, 0] = 7
    with pytest.raises(ValueError):
        R.evaluate(gt, rows)


def test_summary_text_and_stats_from_arrays():
    from multipathnet_amd import cocoeval
    gt, rows = kat1()
    ev = R.evaluate(gt, rows)
    st = cocoeval.summarize_stats(ev["precision"], ev["recall"])
    assert np.array_equal(st, R.summarize(ev["precision"], ev["recall"]))
    txt = cocoeval.summary_text(st).split("\n")
    assert len(txt) == 12
    assert txt[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.450"
    assert txt[1] == " Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = 1.000"
    assert txt[4] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=medium | maxDets=100 ] = -1.000"
    assert txt[6] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.100"
    assert txt[11] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = -1.000"


def test_load_coco_gt_keeps_annotation_order():
    from multipathnet_amd import cocoeval
    ds = {"images": [{"id": 9}, {"id": 3}], "categories": [{"id": 18}, {"id": 1}],
          "annotations": [{"id": 5, "image_id": 9, "category_id": 18, "bbox": [1.5, 2, 3, 4], "area": 11.25, "iscrowd": 0},
                          {"id": 2, "image_id": 3, "category_id": 1, "bbox": [0, 0, 10, 10], "area": 70.0, "iscrowd": 1, "ignore": 0},
                          {"id": 900100000000, "image_id": 9, "category_id": 1, "bbox": [5, 5, 1, 1], "area": 1}]}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        gt = cocoeval.load_coco_gt(ds)
    assert gt["id"].tolist() == [5, 2, 900100000000] and gt["id"].dtype == np.int64
    assert gt["img_ids"].tolist() == [3, 9] and gt["cat_ids"].tolist() == [1, 18]
    assert gt["bbox"].dtype == np.float64 and gt["bbox"][0].tolist() == [1.5, 2, 3, 4]
    assert gt["area"].tolist() == [11.25, 70.0, 1.0] and gt["iscrowd"].tolist() == [0, 1, 0]
    ds["annotations"][0]["id"] = 0
    with pytest.warns(UserWarning, match="id 0"):
        cocoeval.load_coco_gt(ds)


def test_coco_eval_abi_rejects_bad_arguments_without_a_device():
    import multipathnet_amd
    lib = multipathnet_amd.load()
    lib.mpn_last_error.restype = C.c_char_p
    i64, f64 = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    box = np.zeros((1, 4)); area = np.ones(1); z = np.zeros(1, np.int64); ids = np.array([1], np.int64)
    thr = R.IOU_THRS.copy(); rec = R.REC_THRS.copy(); rng = R.AREA_RNG.copy()
    md = (C.c_int * 3)(1, 10, 100)
    p = lambda a, t: a.ctypes.data_as(t)

    def create(**kw):
        a = dict(device=-1, bbox=p(box, f64), area=p(area, f64), crowd=p(z, i64), img=p(ids, i64), cat=p(ids, i64), gid=p(ids, i64),
                 n_gt=1, img_ids=p(ids, i64), n_img=1, ev=None, n_ev=0, cat_ids=p(ids, i64), n_cat=1, thr=p(thr, f64), n_thr=10,
                 rec=p(rec, f64), n_rec=101, rng=p(rng, f64), n_rng=4, md=md, n_md=3)
        a.update(kw)
        h = C.c_void_p()
        rc = lib.mpn_coco_eval_create(*a.values(), C.byref(h))
        return rc, h

    bad = [dict(bbox=None), dict(n_gt=-1), dict(n_img=0), dict(img_ids=None), dict(n_cat=0), dict(n_thr=0), dict(n_thr=17),
           dict(n_rng=9), dict(md=(C.c_int * 3)(1, 10, 0)), dict(md=(C.c_int * 3)(1, 10, 5000)), dict(ev=None, n_ev=3),
           dict(img_ids=p(np.array([4, 4], np.int64), i64), n_img=2), dict(cat_ids=p(np.array([9, 2], np.int64), i64), n_cat=2),
           dict(thr=p(np.full(10, np.nan), f64)), dict(bbox=p(np.full((1, 4), np.inf), f64))]
    for kw in bad:
        rc, h = create(**kw)
        assert rc == -1 and not h.value, kw
        assert b"invalid argument" in lib.mpn_last_error(), kw
    assert lib.mpn_coco_eval_create(*([None] * 22), None) == -1
    f64n = C.POINTER(C.c_double)()
    assert lib.mpn_coco_eval_run(None, None, 0, f64n, f64n, f64n, None) == -1
    assert b"invalid argument" in lib.mpn_last_error()
    lib.mpn_coco_eval_destroy.restype = None
    lib.mpn_coco_eval_destroy(None)                    # destroying nothing is a no-op
