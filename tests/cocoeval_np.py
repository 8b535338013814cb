"""A numpy restatement of pycocotools 2.0's COCOeval for iouType='bbox' (coco.py loadRes, cocoeval.py, maskApi.c bbIou), as
testCoco/coco.lua:24-37 drives it.  Test infrastructure only: never imported by the package.  The contract it restates is
DESIGN.md section 10; the device path (multipathnet_amd.cocoeval) must equal it bit for bit.

gt is the dict multipathnet_amd.cocoeval.load_coco_gt returns: img_ids / cat_ids (sorted int64), and per annotation in file
order bbox [G,4] f64, area f64, iscrowd, image_id, category_id, id (int64)."""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNG = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], np.float64)
AREA_LBL = ["all", "small", "medium", "large"]
MAX_DETS = [1, 10, 100]


def bb_iou(d, g, crowd):
    """maskApi.c bbIou for one pair, in its operation order (python floats are IEEE doubles)."""
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    da = d[2] * d[3]
    u = da if crowd else da + g[2] * g[3] - i
    return i / u


def evaluate(gt, rows, img_ids=None, iou_thrs=IOU_THRS, rec_thrs=REC_THRS, area_rng=AREA_RNG, max_dets=MAX_DETS):
    """-> dict(precision [T,R,K,A,M], recall [T,K,A,M], scores [T,R,K,A,M]) (float64, -1 where undefined)."""
    rows = np.asarray(rows, np.float32).reshape(-1, 7)
    gt_imgs = set(int(v) for v in gt["img_ids"])
    d_img = [int(v) for v in rows[:, 0]]
    d_cat = [int(v) for v in rows[:, 6]]
    if not set(d_img) <= gt_imgs:
        raise ValueError("Results do not correspond to current coco set")          # loadRes's assert
    imgs = sorted(set(d_img)) if img_ids is None else sorted(set(int(v) for v in img_ids))
    cats = sorted(int(v) for v in gt["cat_ids"])
    T, R, K, A, M = len(iou_thrs), len(rec_thrs), len(cats), len(area_rng), len(max_dets)
    ii, kk = {v: i for i, v in enumerate(imgs)}, {v: k for k, v in enumerate(cats)}
    gts, dts = {}, {}
    for g in range(len(gt["id"])):
        key = (int(gt["image_id"][g]), int(gt["category_id"][g]))
        if key[0] in ii and key[1] in kk:
            gts.setdefault(key, []).append(g)
    for r in range(rows.shape[0]):
        key = (d_img[r], d_cat[r])
        if key[0] in ii and key[1] in kk:
            dts.setdefault(key, []).append(r)
    max_det = max_dets[-1]
    thr = [min(float(t), 1 - 1e-10) for t in iou_thrs]
    # evaluateImg for every (k, a, i); None for an empty cell
    E = {}
    for k, cat in enumerate(cats):
        for i, img in enumerate(imgs):
            g, d = gts.get((img, cat), []), dts.get((img, cat), [])
            if not g and not d:
                continue
            sc = rows[d, 5]
            order = np.argsort(-sc, kind="mergesort")[:max_det]
            d = [d[j] for j in order]
            dbox = [[float(rows[r, 1]), float(rows[r, 2]), float(rows[r, 3]), float(rows[r, 4])] for r in d]
            darea = [np.float32(rows[r, 3]) * np.float32(rows[r, 4]) for r in d]
            gbox = [[float(x) for x in gt["bbox"][j]] for j in g]
            crowd = [int(gt["iscrowd"][j]) for j in g]
            ious = [[bb_iou(db, gb, c) for gb, c in zip(gbox, crowd)] for db in dbox]
            for a in range(A):
                lo, hi = float(area_rng[a][0]), float(area_rng[a][1])
                g_ig = [1 if (crowd[j] or float(gt["area"][g[j]]) < lo or float(gt["area"][g[j]]) > hi) else 0 for j in range(len(g))]
                gtind = list(np.argsort(g_ig, kind="mergesort"))
                gig = [g_ig[j] for j in gtind]
                gcr = [crowd[j] for j in gtind]
                gid = [int(gt["id"][g[j]]) for j in gtind]
                D, G = len(d), len(g)
                dtm = np.zeros((T, D), np.int64)
                dtig = np.zeros((T, D), bool)
                if D and G:
                    for t in range(T):
                        gtm = [0] * G
                        for di in range(D):
                            iou, m = thr[t], -1
                            for gi in range(G):
                                if gtm[gi] > 0 and not gcr[gi]:
                                    continue
                                if m > -1 and gig[m] == 0 and gig[gi] == 1:
                                    break
                                v = ious[di][gtind[gi]]
                                if v < iou:
                                    continue
                                iou, m = v, gi
                            if m == -1:
                                continue
                            dtig[t, di] = gig[m]
                            dtm[t, di] = gid[m]
                            gtm[m] = d[di] + 1
                out = np.array([float(x) < lo or float(x) > hi for x in darea], bool).reshape(1, D)
                dtig = np.logical_or(dtig, np.logical_and(dtm == 0, np.repeat(out, T, 0)))
                E[k, a, i] = dict(dtScores=rows[d, 5].astype(np.float32), dtm=dtm, dtig=dtig, gtig=np.array(gig, np.int64))
    return accumulate(E, K, A, len(imgs), rec_thrs, max_dets, T)


def accumulate(E, K, A, I, rec_thrs, max_dets, T):
    R, M = len(rec_thrs), len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    for k in range(K):
        for a in range(A):
            Es = [E[k, a, i] for i in range(I) if (k, a, i) in E]
            if not Es:
                continue
            for m, max_det in enumerate(max_dets):
                dt_scores = np.concatenate([e["dtScores"][0:max_det] for e in Es])
                inds = np.argsort(-dt_scores, kind="mergesort")
                dss = dt_scores[inds]
                dtm = np.concatenate([e["dtm"][:, 0:max_det] for e in Es], axis=1)[:, inds]
                dtig = np.concatenate([e["dtig"][:, 0:max_det] for e in Es], axis=1)[:, inds]
                npig = np.count_nonzero(np.concatenate([e["gtig"] for e in Es]) == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dtig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtig))
                tp_sum = np.cumsum(tps, axis=1).astype(np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(np.float64)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q, ss = np.zeros((R,)), np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = np.maximum.accumulate(pr[::-1])[::-1] if nd else pr
                    pi = np.searchsorted(rc, rec_thrs, side="left")
                    ok = pi < nd
                    q[ok] = pr[pi[ok]]
                    ss[ok] = dss[pi[ok]]
                    precision[t, :, k, a, m] = q
                    scores[t, :, k, a, m] = ss
    return dict(precision=precision, recall=recall, scores=scores)


def summarize(precision, recall, iou_thrs=IOU_THRS, max_dets=MAX_DETS):
    """COCOeval.summarize's 12 numbers (cocoeval.py _summarizeDets)."""
    def one(ap, iou_thr=None, area="all", md=100):
        aind = [i for i, lbl in enumerate(AREA_LBL) if lbl == area]
        mind = [i for i, v in enumerate(max_dets) if v == md]
        if ap:
            s = precision
            if iou_thr is not None:
                s = s[np.where(iou_thr == iou_thrs)[0]]
            s = s[:, :, :, aind, mind]
        else:
            s = recall
            if iou_thr is not None:
                s = s[np.where(iou_thr == iou_thrs)[0]]
            s = s[:, :, aind, mind]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))
    md = max_dets
    return np.array([one(1), one(1, .5, md=md[2]), one(1, .75, md=md[2]), one(1, area="small", md=md[2]), one(1, area="medium", md=md[2]),
                     one(1, area="large", md=md[2]), one(0, md=md[0]), one(0, md=md[1]), one(0, md=md[2]), one(0, area="small", md=md[2]),
                     one(0, area="medium", md=md[2]), one(0, area="large", md=md[2])])


COCO_CAT_IDS = [i for i in range(1, 91) if i not in (12, 26, 29, 30, 45, 66, 68, 69, 71, 83)]   # COCO's 80 ids, gaps included


def synthetic(seed, n_img, cat_ids, gt_per_img=7.3, det_per_img=100, crowd=0.01, hard=False):
    """A seeded GT set (load_coco_gt layout) and fp32 result rows.  About half the detections jitter a GT box (so they match), the
    rest are random; GT `area` is drawn independently of the box (as a segmentation area is).  hard=True adds the corner cases:
    1/64-quantised scores with -0.0 / 0.0, duplicated GT and detection boxes (equal-IoU ties), GT areas exactly on 32^2 and 96^2,
    images with detections and no GT, GT-only images, a category with GT and no detections, a cell with 150 detections and a
    cell with 300 GTs."""
    rng = np.random.default_rng(seed)
    cat_ids = np.asarray(cat_ids, np.int64)
    img_ids = np.sort(rng.choice(np.arange(1, 50 * n_img), n_img, replace=False)).astype(np.int64)
    n_gt_imgs = n_img - 10 if hard else n_img
    counts = rng.poisson(gt_per_img, n_gt_imgs)
    g_img = np.repeat(img_ids[:n_gt_imgs], counts)
    G = g_img.size
    g_cat = rng.choice(cat_ids, G)
    xy = rng.uniform(0, 600, (G, 2))
    wh = np.exp(rng.uniform(np.log(4), np.log(300), (G, 2)))
    if hard:
        dup = rng.random(G) < 0.05                                # duplicated GT boxes: equal IoU, the later GT wins
        xy[1:][dup[1:]] = xy[:-1][dup[1:]]
        wh[1:][dup[1:]] = wh[:-1][dup[1:]]
        g_cat[1:][dup[1:]] = g_cat[:-1][dup[1:]]
        g_img[1:][dup[1:] & (g_img[1:] != g_img[:-1])] = g_img[:-1][dup[1:] & (g_img[1:] != g_img[:-1])]
    bbox = np.round(np.concatenate([xy, wh], 1), 2)
    area = np.round(bbox[:, 2] * bbox[:, 3] * rng.uniform(0.3, 1.0, G), 2)
    if hard:
        b = rng.random(G)
        area[b < 0.05] = 32.0 ** 2
        area[(b >= 0.05) & (b < 0.1)] = 96.0 ** 2
    iscrowd = (rng.random(G) < crowd).astype(np.int64)
    if hard:                                                      # a cell with 300 GTs (matched bits outside LDS)
        k = 300
        g_img = np.concatenate([g_img, np.full(k, img_ids[1])])
        g_cat = np.concatenate([g_cat, np.full(k, cat_ids[1])])
        bb = np.round(np.concatenate([rng.uniform(0, 600, (k, 2)), np.exp(rng.uniform(np.log(8), np.log(120), (k, 2)))], 1), 2)
        bbox = np.concatenate([bbox, bb])
        area = np.concatenate([area, np.round(bb[:, 2] * bb[:, 3], 2)])
        iscrowd = np.concatenate([iscrowd, (rng.random(k) < crowd).astype(np.int64)])
        G = g_img.size
    ids = rng.permutation(np.arange(1, 3 * G + 1))[:G].astype(np.int64)
    gt = {"bbox": bbox.astype(np.float64), "area": area.astype(np.float64), "iscrowd": iscrowd, "image_id": g_img.astype(np.int64),
          "category_id": g_cat.astype(np.int64), "id": ids, "img_ids": img_ids, "cat_ids": np.sort(cat_ids)}
    # detections: per image, jittered copies of its GTs, then random boxes
    n_det_imgs = n_img - 5 if hard else n_img                     # hard: the last 5 images (no GT either) have no rows
    rows = []
    g_of = {}
    for j, im in enumerate(g_img):
        g_of.setdefault(int(im), []).append(j)
    for im in img_ids[:n_det_imgs]:
        gs = g_of.get(int(im), [])
        nd = det_per_img
        take = rng.choice(gs, min(len(gs), nd // 2), replace=False) if gs else np.zeros(0, int)
        jit = bbox[take] * (1 + rng.normal(0, 0.08, (take.size, 4)))
        rnd = np.concatenate([rng.uniform(0, 600, (nd - take.size, 2)), np.exp(rng.uniform(np.log(4), np.log(300), (nd - take.size, 2)))], 1)
        boxes = np.concatenate([jit, rnd])
        cats = np.concatenate([g_cat[take], rng.choice(cat_ids, nd - take.size)])
        sc = rng.random(nd)
        rows.append(np.concatenate([np.full((nd, 1), im), boxes, sc[:, None], cats[:, None]], 1))
    rows = np.concatenate(rows).astype(np.float32)
    if hard:
        rows[:, 5] = np.round(rows[:, 5] * 64) / 64                 # heavy ties
        z = rng.random(rows.shape[0])
        rows[z < 0.02, 5] = -0.0
        rows[(z >= 0.02) & (z < 0.04), 5] = 0.0
        dup = np.flatnonzero(rng.random(rows.shape[0]) < 0.05)      # duplicated detections (same box and score)
        rows = np.concatenate([rows, rows[dup]])
        rows = rows[rows[:, 6] != cat_ids[-1]]                      # a category with GT and no detections
        rows = rows[~np.isin(rows[:, 0], img_ids[2:5].astype(np.float32))]   # GT-only images (only img_ids="all" evaluates them)
        extra = np.concatenate([np.full((150, 1), img_ids[0]), rng.uniform(0, 600, (150, 2)),
                                np.exp(rng.uniform(np.log(8), np.log(200), (150, 2))), np.round(rng.random((150, 1)) * 16) / 16,
                                np.full((150, 1), cat_ids[0])], 1).astype(np.float32)  # a cell with 150 detections
        rows = np.concatenate([rows, extra])
        rows = rows[rng.permutation(rows.shape[0])]
    return gt, rows
