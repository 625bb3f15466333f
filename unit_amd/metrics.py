"""Detectron2's per-step training scalars from counts made on the device (csrc/metrics.hip).

The reference's step feeds its event storage from four places, each with a host sync per scalar:
  rpn/num_pos_anchors, rpn/num_neg_anchors                           modeling/proposal_generator/rpn.py:61-66
  roi_head/num_fg_samples, roi_head/num_bg_samples                   Detectron2 v0.3 ROIHeads.label_and_sample_proposals (roi_heads.py:563)
  fast_rcnn/cls_accuracy, fg_cls_accuracy, false_negative            Detectron2 v0.3 FastRCNNOutputs._log_accuracy (fast_rcnn.py:438-445)
  mask_rcnn/accuracy, false_positive, false_negative                 Detectron2 v0.3 mask_rcnn_loss (mask_head.py:34)
All ten are ratios of integer counts. With `model.collect_metrics = True` the fused step adds the counts into one int32[16] vector
(`model.last_metrics`) without a sync; this module names its slots and does Detectron2's arithmetic on a host copy, in Python floats.
Each process reports its own batch, as Detectron2's per-process storage does: there is no cross-rank averaging here.

Not covered: the mask keys under MaskRCNNConvUpsampleHeadWithFineTune (its gt-class logit exists only inside unit_mask_bce_loss_ft: the keys
are absent there, not approximated) and the module-level training nodes of modeling/train_modules.py.
"""

SIZE = 16
# name -> offset in the vector. Three blocks of five, one per kernel (unit_metrics_rpn uses the first two of its block).
SLOTS = {
    "rpn_pos": 0, "rpn_neg": 1,
    "roi_instances": 5, "roi_correct": 6, "roi_fg": 7, "roi_fg_correct": 8, "roi_fg_as_bg": 9,
    "mask_elements": 10, "mask_incorrect": 11, "mask_positive": 12, "mask_false_positive": 13, "mask_false_negative": 14,
}
RPN, FAST_RCNN, MASK = 0, 5, 10          # first slot of each kernel's block

KEYS = ("rpn/num_pos_anchors", "rpn/num_neg_anchors", "roi_head/num_fg_samples", "roi_head/num_bg_samples", "fast_rcnn/cls_accuracy",
        "fast_rcnn/fg_cls_accuracy", "fast_rcnn/false_negative", "mask_rcnn/accuracy", "mask_rcnn/false_positive", "mask_rcnn/false_negative")


def scalars(raw, n_sup_images):
    """raw: the 16 counts as a sequence of ints (a host copy of `model.last_metrics`); n_sup_images: supervised images of that step.
    -> {Detectron2 key: float}. A key Detectron2 would not have logged for this batch is absent, not zero."""
    v = [int(x) for x in raw]
    assert len(v) == SIZE, f"expected {SIZE} counts, got {len(v)}"
    g = lambda name: v[SLOTS[name]]
    out = {}
    n = int(n_sup_images)
    if n > 0:          # (a step without a supervised batch runs neither the RPN losses nor the RoI sampler)
        out["rpn/num_pos_anchors"] = g("rpn_pos") / n
        out["rpn/num_neg_anchors"] = g("rpn_neg") / n
        # np.mean of the per-image counts: every image contributes one entry, so the mean is the total over the number of images
        out["roi_head/num_fg_samples"] = g("roi_fg") / n
        out["roi_head/num_bg_samples"] = (g("roi_instances") - g("roi_fg")) / n
    if g("roi_instances") > 0:
        out["fast_rcnn/cls_accuracy"] = g("roi_correct") / g("roi_instances")
        if g("roi_fg") > 0:
            out["fast_rcnn/fg_cls_accuracy"] = g("roi_fg_correct") / g("roi_fg")
            out["fast_rcnn/false_negative"] = g("roi_fg_as_bg") / g("roi_fg")
    if g("mask_elements") > 0:          # mask_rcnn_loss returns before logging when no foreground slot reached it
        el, pos = g("mask_elements"), g("mask_positive")
        out["mask_rcnn/accuracy"] = 1 - g("mask_incorrect") / max(el, 1.0)
        out["mask_rcnn/false_positive"] = g("mask_false_positive") / max(el - pos, 1.0)
        out["mask_rcnn/false_negative"] = g("mask_false_negative") / max(pos, 1.0)
    return out


def put_scalars(storage, raw, n_sup_images):
    """feeds an event storage (anything with Detectron2's `put_scalar(name, value)`) with the scalars of one step; returns them"""
    d = scalars(raw, n_sup_images)
    for k, val in d.items():
        storage.put_scalar(k, val)
    return d
