"""Host side of training the Fast R-CNN head (file:line relative to the reference tree): which ROIs enter a minibatch and the
statistics of their regression targets.  numpy / torch on the host, not on the per-image path; the per-step work — frozen trunk, ROI
pooling, head forward, loss, backward, SGD — is models.FastRCNN.train_add / train_step on the device.

  attach_proposals        DataSetJSON.lua:280-390  (DataSetCOCO:attachProposals with its crowd branch, without the sample-around-GT one)
  RoiSampler              BatchProviderROI.lua:39-49 (setupOne), BatchProviderBase.lua:54-107 (takeSubset, selectBBoxesOne)
  attach_proposals_device, DeviceRoiSampler   the same two on the device (mpn_attach_proposals / mpn_sample_rois, DESIGN.md section
                          13.11): what FastRCNN.train_add_sampled / tower_train_add_sampled run per image, with a counter-based draw
  IntegralSampler         donkey.lua:38-41 (the integral loss: one RoiSampler per classifier, each with its own foreground threshold)
  bbox_regression_stats   BatchProviderROI.lua:53-69 (setupData)
  save_checkpoint / load_checkpoint / resume   train.lua:188-198 (model_<epoch>.t7 + optimState_<epoch>.t7, here one table), opt.resume
"""
import ctypes as C

import numpy as np
import torch

from . import t7, utils


def _boxoverlap_host(a, b):
    """utils.boxoverlap (utils.lua:104-128) in fp32 on the host: IoU of a [N,4] with one box b, the +1 pixel convention, 0 where the
    intersection's width or height is negative."""
    a = np.asarray(a, np.float32).reshape(-1, 4)
    b = np.asarray(b, np.float32).reshape(4)
    x1, y1 = np.maximum(a[:, 0], b[0]), np.maximum(a[:, 1], b[1])
    x2, y2 = np.minimum(a[:, 2], b[2]), np.minimum(a[:, 3], b[3])
    w, h = x2 - x1 + np.float32(1), y2 - y1 + np.float32(1)
    inter = w * h
    aarea = (a[:, 2] - a[:, 0] + np.float32(1)) * (a[:, 3] - a[:, 1] + np.float32(1))
    barea = (b[2] - b[0] + np.float32(1)) * (b[3] - b[1] + np.float32(1))
    with np.errstate(divide="ignore", invalid="ignore"):   # a zero union only meets a negative w or h, zeroed below
        o = inter / (aarea + barea - inter)
    o[(w < 0) | (h < 0)] = 0
    return o.astype(np.float32)


def _intersection_host(a, b):
    """utils.intersection (utils.lua:131-148) in fp32 on the host: the share of each box of a [N,4] that lies inside the one box b,
    inter / aarea — WITHOUT boxoverlap's zeroing of negative widths and heights, as the reference writes it: a box off b's corner
    (w < 0 and h < 0) has a positive inter."""
    a = np.asarray(a, np.float32).reshape(-1, 4)
    b = np.asarray(b, np.float32).reshape(4)
    x1, y1 = np.maximum(a[:, 0], b[0]), np.maximum(a[:, 1], b[1])
    x2, y2 = np.minimum(a[:, 2], b[2]), np.minimum(a[:, 3], b[3])
    w, h = x2 - x1 + np.float32(1), y2 - y1 + np.float32(1)
    aarea = (a[:, 2] - a[:, 0] + np.float32(1)) * (a[:, 3] - a[:, 1] + np.float32(1))
    with np.errstate(divide="ignore", invalid="ignore"):   # (a degenerate box of zero area)
        return ((w * h) / aarea).astype(np.float32)


def _to_np(t, dt):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(dt)


def attach_proposals(proposals, gt_boxes, gt_labels, crowd_boxes=None):
    """DataSetCOCO:attachProposals for one image: the GT boxes FIRST, then the proposals (DataSetJSON.lua:291-299); per row the maximum IoU
    with a GT box (`overlap`), the 1-based index of that GT box (`correspondance`, the reference's spelling; the first maximum, 0 where the
    overlap is 0) and its class (`label`, 0 where there is none).  gt_labels are class ids >= 1.  crowd_boxes [k,4] (the image's
    `iscrowd` regions; None or empty: none): a proposal row more than 0.7 inside one of them gets overlap -1 — neither foreground nor
    background —, GT rows never; correspondance and label stay (DataSetJSON.lua:345-363).  Returns a dict of numpy arrays:
    boxes [n,4] float32, gt [n] uint8 (1 on the GT rows), overlap [n] float32, correspondance [n] int64, label [n] int32."""
    prop = _to_np(proposals, np.float32).reshape(-1, 4)
    gtb = _to_np(gt_boxes, np.float32).reshape(-1, 4)
    gtl = _to_np(gt_labels, np.int32).reshape(-1)
    assert gtb.shape[0] == gtl.shape[0]
    ng, n = gtb.shape[0], gtb.shape[0] + prop.shape[0]
    boxes = np.concatenate([gtb, prop], 0)
    rec = {"boxes": boxes, "gt": np.concatenate([np.ones(ng, np.uint8), np.zeros(prop.shape[0], np.uint8)])}
    if ng:
        ov = np.stack([_boxoverlap_host(boxes, gtb[j]) for j in range(ng)], 1) if n else np.zeros((0, ng), np.float32)
        rec["overlap"] = ov.max(1) if n else np.zeros(0, np.float32)
        corr = ov.argmax(1).astype(np.int64) + 1 if n else np.zeros(0, np.int64)   # first maximum, 1-based
        corr[rec["overlap"] == 0] = 0
    else:
        rec["overlap"] = np.zeros(n, np.float32)
        corr = np.zeros(n, np.int64)
    rec["correspondance"] = corr
    label = np.zeros(n, np.int32)
    label[corr > 0] = gtl[corr[corr > 0] - 1]
    rec["label"] = label
    crowds = None if crowd_boxes is None else _to_np(crowd_boxes, np.float32).reshape(-1, 4)
    if crowds is not None and crowds.shape[0] and n:
        mask = np.stack([_intersection_host(boxes, c) for c in crowds], 0).max(0) > np.float32(0.7)
        mask[:ng] = False   # "don't want to exclude ground truth boxes"
        rec["overlap"] = np.where(mask, np.float32(-1), rec["overlap"]).astype(np.float32)
    return rec


def _dev_f32(t, shape=None):
    """a contiguous fp32 device tensor of `t` (numpy, host or device tensor)"""
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(t, np.float32)))
    t = t.to(device="cuda", dtype=torch.float32)
    if shape is not None:
        t = t.reshape((0,) + tuple(shape[1:])) if t.numel() == 0 else t.reshape(shape)   # (-1 cannot be inferred for no elements)
    return t.contiguous()


def _dev_i32(t):
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(t, np.int32)))
    return t.to(device="cuda", dtype=torch.int32).reshape(-1).contiguous()


def _ptr(t):
    return None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def attach_proposals_device(proposals, gt_boxes, gt_labels, crowd_boxes=None):
    """attach_proposals on the device (include/mpn.h mpn_attach_proposals: one launch, the crowd branch included): a record of DEVICE
    tensors boxes [m,4] float32, overlap [m] float32, correspondance [m] int32, label [m] int32, m = g + n, the GT rows first — bit for
    bit what attach_proposals gives.  The inputs may be numpy arrays or tensors on either side."""
    from . import _lib
    lib = _lib.load()
    prop, gtb, gtl = _dev_f32(proposals, (-1, 4)), _dev_f32(gt_boxes, (-1, 4)), _dev_i32(gt_labels)
    crowds = None if crowd_boxes is None else _dev_f32(crowd_boxes, (-1, 4))
    n, g, nc = prop.size(0), gtb.size(0), 0 if crowds is None else crowds.size(0)
    assert gtl.numel() == g
    m, dev = g + n, prop.device
    rec = {"boxes": torch.empty((m, 4), dtype=torch.float32, device=dev), "overlap": torch.empty(m, dtype=torch.float32, device=dev),
           "correspondance": torch.empty(m, dtype=torch.int32, device=dev), "label": torch.empty(m, dtype=torch.int32, device=dev)}
    _lib.check(lib.mpn_attach_proposals(_ptr(prop), n, _ptr(gtb), _ptr(gtl), g, _ptr(crowds), nc, _ptr(rec["boxes"]), _ptr(rec["overlap"]),
                                        _ptr(rec["correspondance"]), _ptr(rec["label"]), _stream()), "mpn_attach_proposals")
    return rec


class DeviceRoiSampler(object):
    """RoiSampler on the device (include/mpn.h mpn_sample_rois): the same two sets and quotas, the draws from
    Philox4x32-10 under (seed, draw) — draw is the caller's counter, one value per (image, minibatch) —, so any host of the C ABI
    reproduces a run's rows.  The integral loss's sampler k is DeviceRoiSampler(batch_size, fg_fraction, t_k, (bg_threshold_min, t_k), seed)
    with IntegralSampler's t_k.  models.FastRCNN.train_add_sampled / tower_train_add_sampled take one of these."""

    def __init__(self, batch_size=128, fg_fraction=0.25, fg_threshold=0.5, bg_threshold=(0.1, 0.5), seed=555):
        self.batch_size, self.fg_fraction = int(batch_size), float(fg_fraction)
        self.fg_threshold, self.bg_threshold = float(fg_threshold), (float(bg_threshold[0]), float(bg_threshold[1]))
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.counts = None   # (n_bg, n_fg) of the last sample()

    def cfg(self):
        """the mpn_roi_sampler this sampler stands for"""
        from . import _lib
        return _lib.RoiSamplerCfg(self.batch_size, self.fg_fraction, self.fg_threshold, self.bg_threshold[0], self.bg_threshold[1])

    def sample(self, rec, draw, flip_width=0):
        """-> (rois [r,4], gt_boxes [r,4], labels [r] int32) device tensors, background rows first (RoiSampler.sample's layout), of an
        attach_proposals_device record; flip_width > 0: both box tables flipped at that image width.  self.counts = (n_bg, n_fg).
        Reads the two counts back (one synchronisation) to cut the tensors to r rows."""
        from . import _lib
        lib = _lib.load()
        boxes, m = rec["boxes"], rec["boxes"].size(0)
        B, dev = self.batch_size, boxes.device
        rois, gt = torch.empty((B, 4), dtype=torch.float32, device=dev), torch.empty((B, 4), dtype=torch.float32, device=dev)
        labels, counts = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(2, dtype=torch.int32, device=dev)
        cfg = self.cfg()
        _lib.check(lib.mpn_sample_rois(_ptr(boxes), _ptr(rec["overlap"]), _ptr(rec["correspondance"]), _ptr(rec["label"]), m, C.byref(cfg),
                                       self.seed, int(draw) & 0xFFFFFFFFFFFFFFFF, int(flip_width), _ptr(rois), _ptr(gt), _ptr(labels),
                                       _ptr(counts), _stream()), "mpn_sample_rois")
        n_bg, n_fg = (int(v) for v in counts.cpu())
        self.counts = (n_bg, n_fg)
        fg_num = int(self.fg_fraction * self.batch_size)
        r = min(self.batch_size - fg_num, n_bg) + min(fg_num, n_fg)
        return rois[:r], gt[:r], labels[:r]


class RoiSampler(object):
    """BatchProviderROI's choice of ROIs for ONE image of a minibatch.  setupOne: foreground = overlap >= fg_threshold, background =
    bg_threshold[0] <= overlap < bg_threshold[1].  selectBBoxesOne: min(num, n) draws WITH replacement from each set, num =
    fg_fraction * batch_size foreground and the rest background PER IMAGE (BatchProviderROI.lua:116-117 — the reference's 128 / 0.25
    are per image; with imgs_per_batch = 2 and 64 rows each pass batch_size = 64).  Background rows first, then foreground
    (BatchProviderROI.lua:98-101).  Labels come out 0-based with 0 = background (the reference's are 1-based)."""

    def __init__(self, batch_size=128, fg_fraction=0.25, fg_threshold=0.5, bg_threshold=(0.1, 0.5), rng=None):
        self.batch_size, self.fg_fraction = int(batch_size), float(fg_fraction)
        self.fg_threshold, self.bg_threshold = float(fg_threshold), (float(bg_threshold[0]), float(bg_threshold[1]))
        self.rng = rng if rng is not None else np.random.default_rng()

    def setup_one(self, rec):
        """(background row indices, foreground row indices) of an attach_proposals record"""
        ov = rec["overlap"]
        fg = np.nonzero(ov >= np.float32(self.fg_threshold))[0]
        bg = np.nonzero((ov >= np.float32(self.bg_threshold[0])) & (ov < np.float32(self.bg_threshold[1])))[0]
        return bg, fg

    def sample(self, rec):
        """-> (rois [m,4] float32, gt_boxes [m,4] float32, labels [m] int32): background rows (gt box zeros, label 0) then foreground
        rows (the GT box each corresponds to, its class)."""
        bg, fg = self.setup_one(rec)
        fg_num = int(self.fg_fraction * self.batch_size)
        bg_num = self.batch_size - fg_num
        pick_bg = bg[self.rng.integers(0, len(bg), min(bg_num, len(bg)))] if len(bg) else bg
        pick_fg = fg[self.rng.integers(0, len(fg), min(fg_num, len(fg)))] if len(fg) else fg
        boxes = rec["boxes"]
        rois = np.concatenate([boxes[pick_bg], boxes[pick_fg]], 0).astype(np.float32)
        gtb = np.concatenate([np.zeros((len(pick_bg), 4), np.float32), boxes[rec["correspondance"][pick_fg] - 1]], 0).astype(np.float32)
        labels = np.concatenate([np.zeros(len(pick_bg), np.int32), rec["label"][pick_fg]]).astype(np.int32)
        return rois, gtb, labels


class IntegralSampler(object):
    """The integral loss's K samplers (donkey.lua:38-41): donkey k, 0-based, draws its ROIs with the foreground threshold
    t_k = bg_threshold_max + k / 20 — foreground = overlap >= t_k, background = bg_threshold_min <= overlap < t_k — and its minibatch
    trains classifier k (FastRCNN.train_set_head(k), train.lua:288-294).  K = 6 at the default 0.5: 0.5, 0.55, ..., 0.75.  The K
    samplers share one generator."""

    def __init__(self, K, batch_size=128, fg_fraction=0.25, bg_threshold_min=0.1, bg_threshold_max=0.5, rng=None):
        self.K = int(K)
        assert self.K >= 1
        rng = rng if rng is not None else np.random.default_rng()
        self.thresholds = [float(bg_threshold_max) + k / 20.0 for k in range(self.K)]
        self.samplers = [RoiSampler(batch_size, fg_fraction, fg_threshold=t, bg_threshold=(bg_threshold_min, t), rng=rng) for t in self.thresholds]

    def sample(self, rec, k):
        """one image's rows for head k: RoiSampler.sample at head k's threshold"""
        return self.samplers[int(k)].sample(rec)


def bbox_regression_stats(records, fg_threshold=0.5):
    """BatchProviderROI:setupData over attach_proposals records: mean and (unbiased, as torch's std) standard deviation of
    utils.convertTo(roi, gt box) over every foreground row -> (mean [4], std [4]) float32 numpy, what FastRCNN takes as
    params["bbox_mean"] / params["bbox_std"]."""
    vals = []
    for rec in records:
        fg = np.nonzero(rec["overlap"] >= np.float32(fg_threshold))[0]
        if len(fg):
            rois = torch.from_numpy(rec["boxes"][fg])
            gtb = torch.from_numpy(rec["boxes"][rec["correspondance"][fg] - 1])
            vals.append(utils.convertTo(rois, gtb))
    assert vals, "no foreground rows"
    v = torch.cat(vals, 0)
    return v.mean(0).numpy(), v.std(0).numpy()


_HEAD_KEYS = ("fc6_w", "fc6_b", "fc7_w", "fc7_b", "cls_w", "cls_b", "bbox_w", "bbox_b")


def save_checkpoint(path, net, epoch=None, learning_rate=None):
    """Everything a training run of a models.FastRCNN or models.MultiPathNet continues from, as ONE Torch7 table (t7.py) — the reference writes the pair
    model_<epoch>.t7 + optimState_<epoch>.t7 (train.lua:188-198).  Between train_begin and train_end.  Flat keys:
      "fc6_w" .. "bbox_b", "conv_w.<l>", "conv_b.<l>"       the weights (net.head_weights() + net.trunk_weights())
      "v.fc6_w" .. "v.bbox_b", "v.conv_w.<l>", "v.conv_b.<l>"  the momentum of every TRAINED tensor (net.train_state(); the others are absent)
      "step", "n_conv", "dropout", "seed"                   the step counter, the trunk's depth, the dropout rate and its seed (a decimal
                                                            string: a Torch7 number is a double, a seed has 64 bits)
      "n_integral"                                          K, only where net holds K > 1 integral classifiers ("cls_w" [K*C, F], "cls_b"
                                                            [K*C] and their momentum stacked in head order): a K = 1 file has no such key
      "epoch", "learningRate"                               only where given: the epoch the file closes and the rate the next one runs at
                                                            (`fit` writes both, behind the rate drop)
    A MultiPathNet net (between tower_train_begin and tower_train_end) gives mpnet_checkpoint_table's keys instead, "kind" = "mpnet"
    among them; a plain file has no "kind"."""
    if torch.cuda.is_available():   # (the copies to the host below wait for the device anyway; a stand-in net in a test has none)
        torch.cuda.synchronize()
    rate, seed = net._dropout
    if getattr(net, "is_mpnet", False):
        tab = mpnet_checkpoint_table(net.tower_weights(), net.tower_train_state(), rate, seed, epoch, learning_rate)
    else:
        Wt = dict(net.head_weights())
        Wt.update(net.trunk_weights())
        tab = plain_checkpoint_table(Wt, net.train_state(), rate, seed, getattr(net, "n_integral", 1), epoch, learning_rate)
    t7.save(path, tab)


def _host(t):
    """a host numpy array of a tensor on either side (or of an array)"""
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _run_keys(tab, rate, seed, step, epoch, learning_rate):
    """what every checkpoint carries beside tensors: the seed as a decimal string (a Torch7 number is a double, a seed has 64 bits)"""
    tab.update({"step": int(step), "dropout": float(rate), "seed": str(int(seed))})
    if epoch is not None:
        tab["epoch"] = int(epoch)
    if learning_rate is not None:
        tab["learningRate"] = float(learning_rate)
    return tab


def plain_checkpoint_table(weights, state, rate, seed, n_integral=1, epoch=None, learning_rate=None):
    """save_checkpoint's table of a plain FastRCNN from plain tensors / arrays on either side (no GPU needed): `weights` =
    head_weights() + trunk_weights(), `state` = train_state()."""
    tab = {k: _host(weights[k]) for k in _HEAD_KEYS}
    n_conv = len(weights["conv_w"])
    for l in range(n_conv):
        tab["conv_w.%d" % l], tab["conv_b.%d" % l] = _host(weights["conv_w"][l]), _host(weights["conv_b"][l])
    for k in _HEAD_KEYS:
        if state[k] is not None:
            tab["v." + k] = _host(state[k])
    for l in range(n_conv):
        if state["conv_w"][l] is not None:
            tab["v.conv_w.%d" % l], tab["v.conv_b.%d" % l] = _host(state["conv_w"][l]), _host(state["conv_b"][l])
    tab["n_conv"] = n_conv
    if n_integral > 1:
        tab["n_integral"] = int(n_integral)
    return _run_keys(tab, rate, seed, state["step"], epoch, learning_rate)


_TOWER_KEYS = ("mix_w", "mix_b", "fc6_w", "fc6_b", "fc7_w", "fc7_b")
_TOWER_GEOMETRY = ("region", "use4", "use3")
_TOWER_HEAD_KEYS = ("cls_w", "cls_b", "bbox_w", "bbox_b")


def mpnet_checkpoint_table(weights, state, rate, seed, epoch=None, learning_rate=None):
    """save_checkpoint's table of a MultiPathNet from plain tensors / arrays on either side (no GPU needed): `weights` = tower_weights(),
    `state` = tower_train_state().  Flat keys:
      "kind" = "mpnet", "n_towers", "n_integral", "n_classes", "n_conv"
      "tower.<t>.mix_w" .. "tower.<t>.fc7_b", "tower.<t>.region" / ".use4" / ".use3"   tower t's weights and its geometry (numbers)
      "cls_w", "cls_b", "bbox_w", "bbox_b"                  the K classifiers stacked, the box regressor
      "conv_w.<l>", "conv_b.<l>"                            the frozen trunk: the reference's model_<n>.t7 holds the whole model
      "bbox_mean", "bbox_std", "conv345_norm"               nn.BBoxNorm's statistics where the net has them; opt.model_conv345_norm
      "v.tower.<t>.<name>", "v.cls_w" .. "v.bbox_b"         the momentum of every trained tensor
      "conv_layers", "v.conv_w.<l>", "v.conv_b.<l>"         only where the run trains conv layers (tower_train_begin(conv_layers=k), k > 0):
                                                            k and the momentum of the trunk's last k layers; a file without them is k = 0
      "step", "dropout", "seed", "epoch", "learningRate"    as in a plain file"""
    tow = weights["towers"]
    tab = {"kind": "mpnet", "n_towers": len(tow), "n_integral": int(weights["n_integral"]), "n_classes": int(weights["n_classes"])}
    for t, T in enumerate(tow):
        for k in _TOWER_KEYS:
            tab["tower.%d.%s" % (t, k)] = _host(T[k])
            tab["v.tower.%d.%s" % (t, k)] = _host(state["towers"][t][k])
        for k in _TOWER_GEOMETRY:
            tab["tower.%d.%s" % (t, k)] = int(T[k])
    for k in _TOWER_HEAD_KEYS:
        tab[k], tab["v." + k] = _host(weights[k]), _host(state[k])
    n_conv = len(weights["conv_w"])
    for l in range(n_conv):
        tab["conv_w.%d" % l], tab["conv_b.%d" % l] = _host(weights["conv_w"][l]), _host(weights["conv_b"][l])
    tab["n_conv"] = n_conv
    for k in ("bbox_mean", "bbox_std"):
        if weights.get(k) is not None:
            tab[k] = np.asarray(_host(weights[k]), np.float64)   # (Python floats at creation: a DoubleTensor keeps them as they are)
    tab["conv345_norm"] = bool(weights.get("conv345_norm", True))
    trained = [l for l, v in enumerate(state.get("conv_w") or []) if v is not None]   # tower_train_begin(conv_layers=k): the last k layers
    if trained:
        tab["conv_layers"] = len(trained)
        for l in trained:
            tab["v.conv_w.%d" % l], tab["v.conv_b.%d" % l] = _host(state["conv_w"][l]), _host(state["conv_b"][l])
    return _run_keys(tab, rate, seed, state["step"], epoch, learning_rate)


def _read_run_keys(tab, out):
    out.update({"dropout": float(tab["dropout"]), "seed": int(tab["seed"])})
    if "epoch" in tab:
        out["epoch"] = int(tab["epoch"])
    if "learningRate" in tab:
        out["learningRate"] = float(tab["learningRate"])
    return out


def checkpoint_read(tab):
    """load_checkpoint behind t7.load: a checkpoint table (as t7.load returns it, or as *_checkpoint_table built it) -> load_checkpoint's
    result with host torch tensors.  A table without "kind" is a plain FastRCNN's."""
    ten = lambda k: torch.from_numpy(np.array(tab[k])) if k in tab else None
    n_conv = int(tab["n_conv"])
    weights = {"conv_w": [ten("conv_w.%d" % l) for l in range(n_conv)], "conv_b": [ten("conv_b.%d" % l) for l in range(n_conv)]}
    if tab.get("kind") == "mpnet":
        nt = int(tab["n_towers"])
        weights["towers"] = []
        state = {"towers": [], "step": int(tab["step"])}
        for t in range(nt):
            T = {k: ten("tower.%d.%s" % (t, k)) for k in _TOWER_KEYS}
            T.update({k: int(tab["tower.%d.%s" % (t, k)]) for k in _TOWER_GEOMETRY})
            T["total_feat"] = int(T["mix_w"].shape[1])
            weights["towers"].append(T)
            state["towers"].append({k: ten("v.tower.%d.%s" % (t, k)) for k in _TOWER_KEYS})
        for k in _TOWER_HEAD_KEYS:
            weights[k], state[k] = ten(k), ten("v." + k)
        weights["n_integral"], weights["n_classes"] = int(tab["n_integral"]), int(tab["n_classes"])
        for k in ("bbox_mean", "bbox_std"):
            if k in tab:
                weights[k] = [float(x) for x in np.asarray(tab[k]).reshape(-1)]
        weights["conv345_norm"] = bool(tab.get("conv345_norm", True))
        k = int(tab.get("conv_layers", 0))
        if k:
            state["conv_w"], state["conv_b"] = [ten("v.conv_w.%d" % l) for l in range(n_conv)], [ten("v.conv_b.%d" % l) for l in range(n_conv)]
        return _read_run_keys(tab, {"kind": "mpnet", "weights": weights, "state": state, "conv_layers": k})
    if "kind" in tab:
        raise ValueError("checkpoint of an unknown kind %r" % (tab["kind"],))
    weights.update({k: ten(k) for k in _HEAD_KEYS})
    if "n_integral" in tab:
        weights["n_integral"] = int(tab["n_integral"])
    state = {k: ten("v." + k) for k in _HEAD_KEYS}
    state["conv_w"], state["conv_b"] = [ten("v.conv_w.%d" % l) for l in range(n_conv)], [ten("v.conv_b.%d" % l) for l in range(n_conv)]
    state["step"] = int(tab["step"])
    return _read_run_keys(tab, {"weights": weights, "state": state})


def load_checkpoint(path):
    """-> {"weights": {...head_weights() keys, "conv_w": [...], "conv_b": [...]}, "state": what FastRCNN.train_load_state takes,
    "dropout": rate, "seed": int} with host torch tensors ("weights" also carries "n_integral" where the file does: K > 1 integral
    classifiers; "epoch" and "learningRate" where the file has them).  Update a parameter dict with "weights" to create the FastRCNN,
    then train_begin (the same depth), train_set_dropout(dropout, seed), train_load_state(state) — or `resume`.
    A MultiPathNet file ("kind" = "mpnet", also returned): "weights" is a dict models.MultiPathNet(...) is built from (tower_weights()'
    keys), "state" what tower_train_load_state takes, "conv_layers" the k the run trains (0 for a file written without it); then
    tower_train_begin(conv_layers=k) and `resume`."""
    return checkpoint_read(t7.load(path))


def resume(net, ckpt):
    """opt.resume: restore load_checkpoint's dropout stream and optimiser state into `net` — a FastRCNN created from ckpt["weights"] on
    which train_begin (the same depth, momentum, weight decay) has been called; or a MultiPathNet created from them on which
    tower_train_begin(conv_layers=ckpt["conv_layers"]) has."""
    if getattr(net, "is_mpnet", False):
        net.tower_train_set_dropout(ckpt["dropout"], ckpt["seed"])
        net.tower_train_load_state(ckpt["state"])
    else:
        net.train_set_dropout(ckpt["dropout"], ckpt["seed"])
        net.train_load_state(ckpt["state"])


def fit(net, batch_fn, n_epochs, epoch_size, lr, step, decay, snapshot=0, save_dir=None, validate=None, log=None, start=None):
    """The epoch loop of train.lua:221-360 (the engine's hooks) on a net that has begun training — train_begin on a plain FastRCNN,
    tower_train_begin on a MultiPathNet; `fit` picks train_* or tower_train_* by net.is_mpnet.  One phase per call (phase2_epoch = -1, the
    shipped recipe): what is trained — the towers alone or, tower_train_begin(conv_layers=k), the trunk's last conv layers with them — is
    what the net has begun; the checkpoints carry k and those layers' momentum.
      batch_fn(epoch, it)   adds minibatch `it` of epoch `epoch` (both 1-based, as in the reference's log lines) to `net` itself with
                            train_add* / tower_train_add*; returns the integral head k the step trains, or None (no set_head call).
                            Which images enter a batch is the caller's: nothing is loaded, decoded or chosen here.
      lr, step, decay       the rate of the first epoch; after every epoch e with e % step == 0: lr *= decay in Python double arithmetic
                            (Lua's), then *_train_scale_momentum(decay) — the reference's dfdx:mul(decay).
      log(dict)             after every epoch, behind the drop: {"epoch", "learningRate", "train_loss", "primary_loss", "bboxregr_loss"},
                            the means over the epoch's steps (train_loss = cls + bbox; the box loss carries bbox_weight).  The steps' two
                            losses are added up on the device and read back once per epoch: no synchronisation per iteration.
      snapshot, save_dir    snapshot > 0: after every epoch e with e % snapshot == 0, save_checkpoint(save_dir/model_<e>.t7) with the epoch
                            and the rate BEHIND the drop, then validate(net, e), whose result is logged as {"epoch", "validate"}.
                            After the last epoch: model_final.t7 and a last validate(net, "final") (save_dir None: nothing is written).
      start                 a load_checkpoint(...) result of such a file: resume(net, start), then epochs start["epoch"] + 1 .. n_epochs at
                            the stored rate.
    With a batch_fn that depends on (epoch, it) alone, a resumed fit gives the bits of the uninterrupted one: the weights, the momentum,
    the step counter and the dropout stream are all in the file.  DeviceRoiSampler makes that easy — its `draw` is a counter the caller
    passes, e.g. draw = ((epoch - 1) * epoch_size + (it - 1)) * images_per_batch + image, with no generator state to carry.
    -> the rate after the last epoch."""
    import os
    mp = bool(getattr(net, "is_mpnet", False))
    set_head, take_step = (net.tower_train_set_head, net.tower_train_step) if mp else (net.train_set_head, net.train_step)
    scale = net.tower_train_scale_momentum if mp else net.train_scale_momentum
    log = log if log is not None else (lambda rec: None)
    lr, first = float(lr), 1
    if start is not None:
        resume(net, start)
        first, lr = int(start["epoch"]) + 1, float(start["learningRate"])

    def save_and_validate(tag, epoch):
        if save_dir is not None:
            save_checkpoint(os.path.join(save_dir, "model_%s.t7" % tag), net, epoch=epoch, learning_rate=lr)
        if validate is not None:
            log({"epoch": epoch, "validate": validate(net, tag)})

    for e in range(first, int(n_epochs) + 1):
        total = None
        for it in range(1, int(epoch_size) + 1):
            k = batch_fn(e, it)
            if k is not None:
                set_head(int(k))
            loss = take_step(lr)
            total = loss if total is None else total + loss   # on the device, in step order
        if e % int(step) == 0:
            lr = lr * float(decay)
            scale(float(decay))
        cls_l, box_l = (float(v) / int(epoch_size) for v in total.cpu())
        log({"epoch": e, "learningRate": lr, "train_loss": cls_l + box_l, "primary_loss": cls_l, "bboxregr_loss": box_l})
        if snapshot and e % int(snapshot) == 0:
            save_and_validate(str(e), e)
    save_and_validate("final", int(n_epochs))
    return lr
