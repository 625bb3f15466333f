"""numpy restatements shared by the TTA fixture generator (tests/golden/gen_tta_golden.py) and the TTA tests: the float32 box rule of the views
(Detectron2's ResizeTransform.apply_box / HFlipTransform.apply_box followed by clip(min=0), meta_arch/rcnn.py:226, :240), the view plan, and
the decision margins of the recorded detections (score threshold, NMS, top-k)."""
import math

import numpy as np

SCALE_CLAMP = math.log(1000.0 / 16)
CASES = ("tta", "tta_ft", "tta_mask", "tta_noflip")
CASE_MODEL = {"tta": "eval", "tta_ft": "eval_ft", "tta_mask": "eval_mask", "tta_noflip": "eval"}
CASE_AUG = {"tta": ((64, 96, 144), 160, True), "tta_ft": ((64, 96, 144), 160, True), "tta_mask": ((96,), 160, True),
            "tta_noflip": ((64, 144), 160, False)}
N_PROPOSALS = 70
MARGIN = 1e-3


def view_plan(h, w, min_sizes, max_size, flip):
    """d2 ResizeShortestEdge.get_transform's size per MIN_SIZES entry, the flipped twin directly behind it -> [(new_h, new_w, flip)...]"""
    plan = []
    for size in min_sizes:
        scale = size * 1.0 / min(h, w)
        newh, neww = (size, scale * w) if h < w else (scale * h, size)
        if max(newh, neww) > max_size:
            scale = max_size * 1.0 / max(newh, neww)
            newh, neww = newh * scale, neww * scale
        nh, nw = int(newh + 0.5), int(neww + 0.5)
        plan.append((nh, nw, False))
        if flip:
            plan.append((nh, nw, True))
    return plan


def view_boxes(boxes, h, w, new_h, new_w, flip, dtype=np.float32):
    """the proposals of one view, in `dtype` arithmetic: x' = x * dtype(new_w / w) (the quotient in double, rounded once), clip(min=0); the
    twin x0'' = dtype(W) - x1', x1'' = dtype(W) - x0', clip(min=0) again. No clip to the maximum."""
    b = np.asarray(boxes, dtype).reshape(-1, 4).copy()
    sx, sy = dtype(new_w * 1.0 / w), dtype(new_h * 1.0 / h)
    b[:, 0::2] = b[:, 0::2] * sx
    b[:, 1::2] = b[:, 1::2] * sy
    b = b.clip(min=0)
    if flip:
        x0 = dtype(new_w) - b[:, 2]
        x1 = dtype(new_w) - b[:, 0]
        b[:, 0], b[:, 2] = x0, x1
        b = b.clip(min=0)
    assert b.dtype == dtype
    return b


def make_proposals(seed, h, w, n=N_PROPOSALS):
    """seeded float32 proposals of an (h, w) image: random boxes, then boxes touching x = 0, boxes touching the right edge and one of zero width"""
    g = np.random.RandomState(seed)
    cx, cy = g.uniform(0.1 * w, 0.9 * w, n), g.uniform(0.1 * h, 0.9 * h, n)
    bw, bh = g.uniform(0.15 * w, 0.6 * w, n), g.uniform(0.15 * h, 0.6 * h, n)
    b = np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1)
    b[:, 0::2] = b[:, 0::2].clip(0, w)
    b[:, 1::2] = b[:, 1::2].clip(0, h)
    b[0:4, 0] = 0.0                      # touching x = 0: the flipped x1 lands on W exactly
    b[4:8, 2] = float(w)                 # touching the right edge: the flipped x0 lands on 0 exactly
    b[8, 2] = b[8, 0]                    # zero width
    return b.astype(np.float32)


def decode(deltas, boxes, weights):
    """Box2BoxTransform.apply_deltas in float32 -> [R, K, 4]"""
    d = np.asarray(deltas, np.float32).reshape(len(boxes), -1, 4)
    b = np.asarray(boxes, np.float32)
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    cx, cy = b[:, 0] + np.float32(0.5) * w, b[:, 1] + np.float32(0.5) * h
    dx, dy = d[..., 0] / np.float32(weights[0]), d[..., 1] / np.float32(weights[1])
    dw = np.minimum(d[..., 2] / np.float32(weights[2]), np.float32(SCALE_CLAMP))
    dh = np.minimum(d[..., 3] / np.float32(weights[3]), np.float32(SCALE_CLAMP))
    pcx, pcy = dx * w[:, None] + cx[:, None], dy * h[:, None] + cy[:, None]
    pw, ph = np.exp(dw) * w[:, None], np.exp(dh) * h[:, None]
    half = np.float32(0.5)
    return np.stack([pcx - half * pw, pcy - half * ph, pcx + half * pw, pcy + half * ph], -1).astype(np.float32)


def _iou(a, b):
    xx1, yy1 = np.maximum(a[0], b[:, 0]), np.maximum(a[1], b[:, 1])
    xx2, yy2 = np.minimum(a[2], b[:, 2]), np.minimum(a[3], b[:, 3])
    inter = np.maximum(xx2 - xx1, 0) * np.maximum(yy2 - yy1, 0)
    union = (a[2] - a[0]) * (a[3] - a[1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - inter
    return np.where(union > 0, inter / np.where(union > 0, union, 1), 0.0)


def detection_margins(probs_sum, delta_mean, props, image_size, weights=(10.0, 10.0, 5.0, 5.0), score_thresh=0.05, nms_thresh=0.5, topk=100):
    """fast_rcnn_inference on the combined predictions, in double on float32 inputs, recording how far every decision is from flipping:
    -> dict(score = min relative distance of a (RoI, class) score from the threshold, iou = min distance of a deciding NMS IoU from the
    threshold, topk = relative gap between the last kept and the first dropped score (inf when nothing is dropped), n = detections)"""
    p = np.asarray(probs_sum, np.float64)[:, :-1]
    r, k = p.shape
    boxes = decode(delta_mean, props, weights).astype(np.float64)
    h, w = image_size
    boxes[..., 0::2] = boxes[..., 0::2].clip(0, w)
    boxes[..., 1::2] = boxes[..., 1::2].clip(0, h)
    m_score = float(np.min(np.abs(p - score_thresh) / score_thresh))
    ri, ci = np.nonzero(p > score_thresh)
    sc, bb = p[ri, ci], boxes[ri, ci]
    order = np.argsort(-sc, kind="stable")
    sc, bb, cls = sc[order], bb[order], ci[order]
    m_iou, kept = np.inf, []
    for j in range(len(sc)):          # per-class NMS (batched_nms): a candidate meets the kept boxes of its own class only
        same = [i for i in kept if cls[i] == cls[j]]
        worst = float(np.max(_iou(bb[j], bb[same]))) if same else 0.0
        # the decision is the maximum IoU against the threshold: that is the quantity whose distance matters
        m_iou = min(m_iou, abs(worst - nms_thresh)) if same else m_iou
        if worst <= nms_thresh:
            kept.append(j)
    m_topk = np.inf
    if len(kept) > topk:
        a, b = sc[kept[topk - 1]], sc[kept[topk]]
        m_topk = float((a - b) / a)
    return dict(score=m_score, iou=float(m_iou), topk=m_topk, n=min(len(kept), topk))
