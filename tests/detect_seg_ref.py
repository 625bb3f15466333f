"""Host restatement of the class-segmented NMS stage (unit_detection_class_segments -> unit_nms per class -> unit_detection_merge_keep),
built on the oracle's `nms`: shift as the kernel does, per-class NMS, merge by the global stable score order, cut at topk. No arithmetic of
its own but the shift, which is batched_nms's. Every function works on ONE image's candidate list in (RoI, class) order."""
import torch

import unit_oracle as orc


def host_candidates(probs, deltas, props, pcount, image_hw, score_thresh, weights):
    """the first half of fast_rcnn_inference_single per image, without the NMS: (boxes [n,4] clipped, scores [n], classes [n] int64, roi [n]
    int64 ORIGINAL rows) in (RoI, class) order -- what dc.candidates reads back through an NMS that suppresses nothing (quadratic: not for
    72 000 candidates)"""
    b, rcap = props.shape[0], props.shape[1]
    out = []
    for i in range(b):
        n = min(int(pcount[i]), rcap)
        rows = slice(i * rcap, i * rcap + n)
        boxes = orc.apply_deltas(deltas[rows], props[i, :n], weights)
        sc = probs[rows]
        valid = torch.isfinite(boxes).all(dim=1) & torch.isfinite(sc).all(dim=1)
        rows_kept = valid.nonzero()[:, 0]
        boxes, sc = boxes[valid], sc[valid][:, :-1]
        k = sc.shape[1]
        bx = boxes.reshape(-1, k, 4).clone()
        h, w = float(image_hw[i][0]), float(image_hw[i][1])
        bx[..., 0].clamp_(0, w)
        bx[..., 1].clamp_(0, h)
        bx[..., 2].clamp_(0, w)
        bx[..., 3].clamp_(0, h)
        mask = sc > score_thresh
        inds = mask.nonzero()
        out.append((bx[mask], sc[mask], inds[:, 1], rows_kept[inds[:, 0]]))
    return out


def score_order(scores):
    """(order, pos): the stable descending score order of the candidates and each candidate's position in it"""
    order = torch.sort(scores, descending=True, stable=True)[1]
    pos = torch.empty_like(order)
    pos[order] = torch.arange(order.numel())
    return order, pos


def shifted(boxes, classes):
    """batched_nms's coordinate shift, float32: class * (max_coordinate + 1)"""
    off = classes.to(boxes) * (boxes.max() + 1)
    return boxes + off[:, None]


def segments(scores, classes, k):
    """per class the candidate indices in descending-score order, ties in (RoI, class) order: what a segment holds, slot by slot"""
    order, _ = score_order(scores)
    cls_sorted = classes[order]
    return [order[cls_sorted == c] for c in range(k)]


def class_keeps(boxes, scores, classes, k, nms_thresh, topk):
    """per class the kept SLOTS of its segment (ascending), at most topk: unit_nms on that segment with max_keep = topk"""
    if scores.numel() == 0:
        return [torch.empty(0, dtype=torch.int64) for _ in range(k)]
    sh = shifted(boxes, classes)
    out = []
    for members in segments(scores, classes, k):
        # members are in descending score order already; the oracle's stable sort leaves them so
        out.append(orc.nms(sh[members], scores[members], nms_thresh)[:topk])
    return out


def segmented_keep(boxes, scores, classes, k, nms_thresh, topk):
    """kept candidates (indices into the (RoI, class) list) in detection order: the union of the per-class survivors by global position, the
    first topk"""
    if scores.numel() == 0:
        return torch.empty(0, dtype=torch.int64)
    _, pos = score_order(scores)
    segs = segments(scores, classes, k)
    kept = torch.cat([m[s] for m, s in zip(segs, class_keeps(boxes, scores, classes, k, nms_thresh, topk))])
    return kept[torch.argsort(pos[kept])][:topk]


def full_keep(boxes, scores, classes, nms_thresh, topk):
    """the existing rule: the oracle's batched_nms over the whole list, cut at topk"""
    return orc.batched_nms(boxes, scores, classes, nms_thresh)[:topk]


def segmented_detections(cands, k, nms_thresh, topk):
    """per image dict(boxes, scores, classes, roi) as dc.ref_detections lays them out, by the segmented rule on given candidate lists"""
    out = []
    for bx, sc, cls, roi in cands:
        keep = segmented_keep(bx, sc, cls, k, nms_thresh, topk)
        out.append(dict(boxes=bx[keep], scores=sc[keep], classes=cls[keep], roi=roi[keep]))
    return out
