"""numpy float32 restatement of horizontal-flip test-time augmentation (include/mpn.h mpn_frcnn_set_augment):
rule 2 (utils.flipBoxes, utils.lua:151-155), rule 4 (the merge), rule 5's clamp and rule 6's loop around a caller-supplied detect.
Every operation is one float32 numpy operation, so each is rounded on its own and nothing can contract into an FMA."""
import numpy as np

F32 = np.float32


def flip_boxes(boxes, image_width):
    """utils.flipBoxes: x1' = ((-x2) + W) + 1, x2' = ((-x1) + W) + 1, every other column unchanged.  boxes [n, >= 4]."""
    b = np.asarray(boxes, F32)
    w = F32(image_width)
    out = b.copy()
    out[:, 0] = ((-b[:, 2]) + w) + F32(1)
    out[:, 2] = ((-b[:, 0]) + w) + F32(1)
    return out


def hflip(im):
    """rule 1: im_f[c, y, x] = im[c, y, W - 1 - x]"""
    return np.ascontiguousarray(np.asarray(im)[..., ::-1])


def clamp_boxes(bbox, image_width, image_height):
    """Tester_FRCNN.lua:75-78 as the device applies it: v < 1 -> 1, v > hi -> hi, a NaN stays a NaN.  bbox [n, 4C]."""
    out = np.asarray(bbox, F32).copy().reshape(-1, 4)
    for col, hi in ((0, image_width), (2, image_width), (1, image_height), (3, image_height)):
        v = out[:, col].copy()
        out[:, col] = np.where(v < F32(1), F32(1), np.where(v > F32(hi), F32(hi), v))
    return out.reshape(np.asarray(bbox).shape)


def merge(sA, bA, sB, bB, image_width, image_height=None, clamp=False):
    """rule 4: scores = (sA + sB) * 0.5, bbox[:, 4c:4c+4] = (bA_c + flipBoxes(bB_c, W)) * 0.5; rule 5: then the clamp where asked for.
    sA, sB [n, C]; bA, bB [n, 4C] (bB in the mirrored frame)."""
    sA, sB, bA, bB = (np.asarray(t, F32) for t in (sA, sB, bA, bB))
    scores = (sA + sB) * F32(0.5)
    back = flip_boxes(bB.reshape(-1, 4), image_width).reshape(bB.shape)
    bbox = (bA + back) * F32(0.5)
    if clamp:
        bbox = clamp_boxes(bbox, image_width, image_height)
    return scores, bbox


def detect(detect_half, boxes, image_width, image_height=None, clamp=False):
    """rules 2-5 around detect_half(mirrored, boxes) -> (scores, bbox): ImageDetect:detect, unclamped, on the upright image
    (mirrored = False) or on the mirrored one (True; it receives flipBoxes of the boxes and answers in the mirrored frame)."""
    sA, bA = detect_half(False, np.asarray(boxes, F32))
    sB, bB = detect_half(True, flip_boxes(boxes, image_width))
    return merge(sA, bA, sB, bB, image_width, image_height, clamp)


def tester_tables(detect_half, select_boxes, boxes, image_width, image_height, num_iter=1, use_rbox_scores=False):
    """rule 6 (Tester_FRCNN.lua:72-100 around the merged detect): the first pass clamped, pass i + 1 on SelectBoxes of the MERGED
    tables of pass i, unclamped; use_rbox_scores pairs the scores of pass i + 1 with the boxes of pass i.  Returns the score and box
    tables that reach the per-class NMS (the passes' rows one after the other)."""
    all_s, all_b = [], []
    b = np.asarray(boxes, F32)
    for it in range(num_iter):
        s, bb = detect(detect_half, b, image_width, image_height, clamp=(it == 0))
        all_s.append(s)
        all_b.append(bb)
        if it + 1 < num_iter:
            b = np.asarray(select_boxes(s, bb), F32)
    if use_rbox_scores:
        assert len(all_s) > 1   # Tester_FRCNN.lua:92
        all_s, all_b = all_s[1:], all_b[:-1]
    return np.concatenate(all_s), np.concatenate(all_b)
