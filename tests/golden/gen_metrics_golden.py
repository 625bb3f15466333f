"""Generates tests/golden/metrics_golden.npz: the scalars the reference's training step hands to Detectron2's event storage, recorded
while re-running the reference step of gen_ref_step.step_inputs for the cases "s1", "s2", "mask" and "coco_mask".

What runs is the reference's own step (gen_unit_golden.build_reference_model, as for ref_step_golden.npz) with a RECORDING event
storage in place of the inert stub: `get_event_storage` is patched in every loaded reference module (they bound it at import), so
rpn/num_pos_anchors and rpn/num_neg_anchors come straight out of the reference's rpn.py:61-66. The other eight scalars are logged by
Detectron2 code the image does not have; the stubs that stand in for it get the restated v0.3 logging blocks of tests/metrics_ref.py,
from this file, at run time (tests/golden/d2_stubs.py itself is unchanged):
  * FastRCNNOutputs.softmax_cross_entropy_loss calls `_log_accuracy()` first, as v0.3 does, and `_log_accuracy` is metrics_ref.log_accuracy;
  * the sampler stand-in `label_and_sample_proposals` logs roi_head/num_{fg,bg}_samples over its per-image classes;
  * the stand-in `mask_rcnn_loss` logs the accuracy block over the logits and the cropped ground truth it is given.

Before the step the bias of the trainable class scorer is shifted by metrics_ref.CLS_BIAS_SHIFT (the step tests do the same): with the
plain synthetic weights no RoI of any case is classified right and the three fast_rcnn/* scalars would all be 0.0.

Stored per case: the recorded keys and values, the raw counts in unit_amd.metrics.SLOTS order, the number of supervised images, and two
"undecided" counts that bound how far a float implementation of the same step may legitimately differ in its counts: classifier rows whose
top-two logit gap is below 1e-4 * max|finite logit|, and mask elements with |gt-class logit| < 1e-5. Each must stay within 1 % of its
population (asserted here). Numbers only; run here:  python tests/golden/gen_metrics_golden.py [out_dir]
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p_ in (HERE, os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "oracle")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

CASES = ("s1", "s2", "mask", "coco_mask")
OUT = os.path.join(HERE, "metrics_golden.npz")


class RecordingStorage:
    """the part of Detectron2's EventStorage the step touches"""
    iter = 0

    def __init__(self):
        self.scalars, self.raw = {}, {}

    def put_scalar(self, name, value, *a, **k):
        assert name not in self.scalars, f"{name} logged twice in one step"
        self.scalars[name] = float(value)

    def put_image(self, *a, **k):
        pass


def run_case(G, S, R, name):
    import unit_oracle as orc
    from unit_amd import metrics as M
    d2 = G.d2
    storage = RecordingStorage()
    for mod in G.REF.values():
        if hasattr(mod, "get_event_storage"):
            mod.get_event_storage = lambda: storage
    cfg, model, sup, weak, perms, masks = S.step_inputs(name)
    K = cfg.MODEL.ROI_HEADS.NUM_CLASSES
    R.shift_classifier_bias(model, name)          # (so that the classifier scalars are not all 0.0: metrics_ref.CLS_BIAS_SHIFT)
    p = S.oracle_params(model)
    ocfg = S.oracle_cfg(cfg)
    if K == 80:
        d2._MetadataCatalog.table["coco_base_training_query_train"] = d2._Metadata(S.COCO_THING_CLASSES)
    mask_cls = cfg.MODEL.ROI_MASK_HEAD.NAME if cfg.MODEL.MASK_ON else None
    ref, trace = G.build_reference_model(p, ocfg, perms, roi_cls=cfg.MODEL.ROI_HEADS.NAME, pred_cls=cfg.MODEL.ROI_HEADS.FAST_RCNN.NAME,
                                         mask_cls=mask_cls)
    if K == 80:
        ref.roi_heads.train_dataset_name = "coco_base_training_query_train"
        ref.roi_heads._class_mappings()
    ref.roi_heads.visual_threshold = ocfg["visual_threshold"]
    ref.roi_heads.box_predictor._freeze_layers(list(cfg.MODEL.FREEZE_LAYERS.FAST_RCNN))
    counts = np.zeros(M.SIZE, np.int64)
    und = {"rows": 0, "row_population": 0, "elements": 0, "element_population": 0}

    # ---- FastRCNNOutputs (stub): v0.3's softmax_cross_entropy_loss logs before it computes the loss
    def _log_accuracy(self):
        c5, sc = R.log_accuracy(self.pred_class_logits.detach(), self.gt_classes)
        counts[M.FAST_RCNN:M.FAST_RCNN + 5] = c5
        lg = self.pred_class_logits.detach()
        top2 = lg.topk(2, dim=1).values
        scale = lg[torch.isfinite(lg)].abs().max().item()
        und["rows"] += int(((top2[:, 0] - top2[:, 1]) < 1e-4 * scale).sum().item())
        und["row_population"] += lg.shape[0]
        for k, v in sc.items():
            storage.put_scalar(k, v)

    def softmax_cross_entropy_loss(self):
        if self._no_instances:
            return 0.0 * self.pred_class_logits.sum()
        self._log_accuracy()
        return F.cross_entropy(self.pred_class_logits, self.gt_classes, reduction="mean")

    saved = (d2.FastRCNNOutputs._log_accuracy, d2.FastRCNNOutputs.softmax_cross_entropy_loss)
    d2.FastRCNNOutputs._log_accuracy, d2.FastRCNNOutputs.softmax_cross_entropy_loss = _log_accuracy, softmax_cross_entropy_loss

    # ---- ROIHeads.label_and_sample_proposals (stand-in built by build_reference_model): v0.3 logs the per-image means
    sampler = ref.roi_heads.label_and_sample_proposals

    def label_and_sample_proposals(proposals, targets):
        res = sampler(proposals, targets)
        c2, sc = R.roi_head_scalars([q.gt_classes for q in res], K)
        counts[M.SLOTS["roi_fg"]] = c2[0]          # (instances come from _log_accuracy; checked against fg + bg below)
        und["roi_bg"] = c2[1]
        for k, v in sc.items():
            storage.put_scalar(k, v)
        return res
    ref.roi_heads.label_and_sample_proposals = label_and_sample_proposals

    # ---- mask_rcnn_loss (stand-in): v0.3 logs the accuracy block when there is at least one mask
    if mask_cls is not None:
        mm = G.REF["mask_head"]
        inner = mm.mask_rcnn_loss

        def mask_rcnn_loss(logits, instances, vis_period=0):
            if logits.shape[0] > 0:
                gcls = torch.cat([i.gt_classes for i in instances])
                tg = torch.cat([orc.crop_and_resize_bitmasks(i.gt_masks, i.proposal_boxes.tensor, logits.shape[-1]) for i in instances], 0)
                c5, sc = R.mask_scalars(logits.detach(), gcls, tg)
                counts[M.MASK:M.MASK + 5] = c5
                gl = logits.detach()[torch.arange(len(gcls)), gcls]
                und["elements"] += int((gl.abs() < 1e-5).sum().item())
                und["element_population"] += gl.numel()
                for k, v in sc.items():
                    storage.put_scalar(k, v)
            return inner(logits, instances, vis_period)
        mm.mask_rcnn_loss = mask_rcnn_loss

    try:
        ref.train()
        losses = ref(G.to_d2_inputs(sup, masks), G.to_d2_inputs(weak) if weak else None)
    finally:
        d2.FastRCNNOutputs._log_accuracy, d2.FastRCNNOutputs.softmax_cross_entropy_loss = saved
    assert all(torch.isfinite(v).all() for v in losses.values())
    n = len(sup)
    counts[M.SLOTS["rpn_pos"]] = round(storage.scalars["rpn/num_pos_anchors"] * n)
    counts[M.SLOTS["rpn_neg"]] = round(storage.scalars["rpn/num_neg_anchors"] * n)
    assert counts[M.SLOTS["roi_instances"]] == counts[M.SLOTS["roi_fg"]] + und["roi_bg"]
    # the recorded scalars are what unit_amd.metrics.scalars makes of the counts (exactly: the same integer ratios in Python floats)
    mine = M.scalars(counts.tolist(), n)
    assert mine == storage.scalars, (mine, storage.scalars)
    for kind in ("rows", "elements"):
        pop = und["row_population" if kind == "rows" else "element_population"]
        assert und[kind] <= 0.01 * pop, f"{name}: {und[kind]} undecided {kind} of {pop} -- choose another seed for this case"
    sl = M.SLOTS
    assert 0 < counts[sl["roi_correct"]] < counts[sl["roi_instances"]], f"{name}: the classifier counts say nothing ({counts.tolist()})"
    keys = sorted(storage.scalars)
    print(name, {k: round(storage.scalars[k], 6) for k in keys}, "undecided", und)
    return {f"{name}/keys": np.array(keys), f"{name}/values": np.array([storage.scalars[k] for k in keys], dtype=np.float64),
            f"{name}/counts": counts, f"{name}/n_images": np.array(n, dtype=np.int64),
            f"{name}/undecided_rows": np.array(und["rows"], dtype=np.int64), f"{name}/rows": np.array(und["row_population"], dtype=np.int64),
            f"{name}/undecided_elements": np.array(und["elements"], dtype=np.int64),
            f"{name}/elements": np.array(und["element_population"], dtype=np.int64)}


def main(out_dir=None):
    import gen_unit_golden as G          # installs the stubs and loads the reference's modules by file
    G.load_meta_arch()
    import gen_ref_step as S
    import metrics_ref as R
    out = {}
    for name in CASES:
        out.update(run_case(G, S, R, name))
    from unit_amd.metrics import SLOTS
    assert any(out[f"{n}/counts"][SLOTS["roi_fg_correct"]] > 0 and out[f"{n}/counts"][SLOTS["roi_fg_as_bg"]] > 0 for n in CASES), \
        "no case has both a foreground hit and a foreground row called background"
    path = OUT if out_dir is None else os.path.join(out_dir, "metrics_golden.npz")
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
