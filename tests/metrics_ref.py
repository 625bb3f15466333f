"""CPU restatement (torch) of the four logging blocks behind the training scalars, for tests/test_metrics_*.py and
tests/golden/gen_metrics_golden.py. Detectron2 is not installed where the tests run; as oracle/unit_oracle.py does for its Detectron2
half, each function cites the source whose arithmetic it restates:

  rpn_scalars          the reference's modeling/proposal_generator/rpn.py:61-66 (WSRPN.losses)
  roi_head_scalars     detectron2/modeling/roi_heads/roi_heads.py, ROIHeads.label_and_sample_proposals (v0.3): num_fg_samples / num_bg_samples
  log_accuracy         detectron2/modeling/roi_heads/fast_rcnn.py, FastRCNNOutputs._log_accuracy (v0.3)
  mask_scalars         detectron2/modeling/roi_heads/mask_head.py, mask_rcnn_loss (v0.3): the accuracy block before the loss

Every function returns (raw integer counts in the kernels' counter order, {key: value}) and computes the values exactly as the cited code
does -- `.item()` ints divided in Python floats. `argmax` is torch.argmax on CPU, the rule unit_metrics_fastrcnn follows.
"""
import numpy as np
import torch


def rpn_scalars(gt_labels):
    """gt_labels: per-image label tensors (1 positive, 0 negative, -1 ignored), as WSRPN.losses receives them. The two scalars are the
    batch's positive / negative anchor counts divided by the number of images."""
    flat = torch.cat([g.reshape(-1) for g in gt_labels])
    pos, neg = int((flat == 1).sum()), int((flat == 0).sum())
    n = len(gt_labels)
    return [pos, neg], {"rpn/num_pos_anchors": pos / n, "rpn/num_neg_anchors": neg / n}


def roi_head_scalars(gt_classes_per_image, num_classes):
    """gt_classes_per_image: the sampled proposals' classes of every image (background = num_classes)"""
    num_fg_samples, num_bg_samples = [], []
    for gt_classes in gt_classes_per_image:
        num_bg_samples.append((gt_classes == num_classes).sum().item())
        num_fg_samples.append(gt_classes.numel() - num_bg_samples[-1])
    return [sum(num_fg_samples), sum(num_bg_samples)], {"roi_head/num_fg_samples": float(np.mean(num_fg_samples)),
                                                        "roi_head/num_bg_samples": float(np.mean(num_bg_samples))}


def log_accuracy(pred_class_logits, gt_classes):
    """pred_class_logits [R, K + 1], gt_classes [R] in [0, K] -> counts [instances, correct, fg, fg correct, fg called background]"""
    num_instances = gt_classes.numel()
    scalars = {}
    if num_instances == 0:          # (argmax of an empty matrix raises; FastRCNNOutputs.losses never logs for an empty batch)
        return [0, 0, 0, 0, 0], scalars
    pred_classes = pred_class_logits.argmax(dim=1)
    bg_class_ind = pred_class_logits.shape[1] - 1
    fg_inds = (gt_classes >= 0) & (gt_classes < bg_class_ind)
    num_fg = fg_inds.nonzero().numel()
    fg_gt_classes = gt_classes[fg_inds]
    fg_pred_classes = pred_classes[fg_inds]
    num_false_negative = (fg_pred_classes == bg_class_ind).nonzero().numel()
    num_accurate = (pred_classes == gt_classes).nonzero().numel()
    fg_num_accurate = (fg_pred_classes == fg_gt_classes).nonzero().numel()
    if num_instances > 0:
        scalars["fast_rcnn/cls_accuracy"] = num_accurate / num_instances
        if num_fg > 0:
            scalars["fast_rcnn/fg_cls_accuracy"] = fg_num_accurate / num_fg
            scalars["fast_rcnn/false_negative"] = num_false_negative / num_fg
    return [num_instances, num_accurate, num_fg, fg_num_accurate, num_false_negative], scalars


def mask_scalars(pred_mask_logits, gt_classes, gt_masks):
    """pred_mask_logits [B, K, M, M], gt_classes [B] in [0, K), gt_masks [B, M, M] bool (already cropped and resized)
    -> counts [elements, incorrect, positives, false positives, false negatives]"""
    total_num_masks = pred_mask_logits.size(0)
    if total_num_masks == 0 or len(gt_masks) == 0:          # mask_rcnn_loss returns `pred_mask_logits.sum() * 0` before it logs
        return [0, 0, 0, 0, 0], {}
    indices = torch.arange(total_num_masks)
    pred_mask_logits = pred_mask_logits[indices, gt_classes]
    gt_masks_bool = gt_masks.to(dtype=torch.bool)
    mask_incorrect = (pred_mask_logits > 0.0) != gt_masks_bool
    num_incorrect = mask_incorrect.sum().item()
    mask_accuracy = 1 - (num_incorrect / max(mask_incorrect.numel(), 1.0))
    num_positive = gt_masks_bool.sum().item()
    num_fp = (mask_incorrect & ~gt_masks_bool).sum().item()
    num_fn = (mask_incorrect & gt_masks_bool).sum().item()
    false_positive = num_fp / max(gt_masks_bool.numel() - num_positive, 1.0)
    false_negative = num_fn / max(num_positive, 1.0)
    return [mask_incorrect.numel(), num_incorrect, num_positive, num_fp, num_fn], {
        "mask_rcnn/accuracy": mask_accuracy, "mask_rcnn/false_positive": false_positive, "mask_rcnn/false_negative": false_negative}


def fastrcnn_counts_with_empty_slots(scores, roi_cls):
    """unit_metrics_fastrcnn's contract on a slot matrix: rows whose class lies outside [0, K] are no instances -- drop them, then
    log_accuracy. -> the five counts"""
    k = scores.shape[1] - 1
    keep = (roi_cls >= 0) & (roi_cls <= k)
    return log_accuracy(scores[keep], roi_cls[keep].long())[0]


def mask_counts_from_layout(logits, k, ldk, cls, targets):
    """unit_metrics_mask's contract: logits fp32 [S * P * P * 4, ldk] in unit_mask_bce_loss's row order (P = M / 2; pixel (Y, X) ->
    [Y/2][X/2][(Y&1)*2 + (X&1)]), cls [S] (outside [0, k): the slot is skipped), targets uint8 [S, M, M] -> the five counts of mask_scalars"""
    s, m = targets.shape[0], targets.shape[-1]
    p = m // 2
    keep = (cls >= 0) & (cls < k)
    if s == 0 or not bool(keep.any()):
        return [0, 0, 0, 0, 0]
    # [S][P][P][2][2][ldk] -> [S][ldk][P][2][P][2] -> [S][ldk][M][M]
    nchw = logits.view(s, p, p, 2, 2, ldk).permute(0, 5, 1, 3, 2, 4).reshape(s, ldk, m, m)[:, :k]
    return mask_scalars(nchw[keep], cls[keep].long(), targets[keep] != 0)[0]


# The synthetic weights of gen_ref_step.step_inputs give every RoI of a case the same one or two predicted classes, none of them a
# ground-truth class: the reference then logs 0.0 for all three fast_rcnn/* scalars and a step test could not tell a right classifier
# count from a wrong one. tests/golden/gen_metrics_golden.py and the step tests therefore shift the bias of the trainable class scorer
# (cls_score_ft in the fine-tune cases, cls_score_delta otherwise) by the SAME fixed amounts, {class column: shift}, before the step:
# the background column by about the median of what the background rows lack, one ground-truth class by more than its rows lack. The
# shifted logits leave every row a top-two gap of at least 0.14 (the reference's logits, fp32), 60 x the "undecided" gap of the generator; the
# generator asserts that every case then has hits and that one case has foreground hits and foreground rows called background.
CLS_BIAS_SHIFT = {
    "s1": {20: 11.5, 16: 5.0},
    "s2": {20: 30.6, 7: 18.0},
    "mask": {20: 8.8, 8: 3.5},
    "mask_ft": {},
    "coco_mask": {80: 7.2},
}


def shift_classifier_bias(model, name):
    """applies CLS_BIAS_SHIFT[name] to the unit_amd model of gen_ref_step.step_inputs(name), in place"""
    from unit_amd.layers import invalidate_prepared
    bp = model.roi_heads.box_predictor
    lin = bp.cls_score_ft if hasattr(bp, "cls_score_ft") else bp.cls_score_delta
    with torch.no_grad():
        for col, shift in CLS_BIAS_SHIFT[name].items():
            lin.bias[col] += shift
    invalidate_prepared()
