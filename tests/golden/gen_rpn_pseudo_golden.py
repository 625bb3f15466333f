"""Generates tests/golden/rpn_pseudo_golden.npz by RUNNING THE REFERENCE'S OWN `WeaklySupervisedRCNNRPN.forward`
(/root/reference/modeling/meta_arch/rcnn.py:544-654) in the authoring container, on the stubbed Detectron2 modules of gen_unit_golden.py
(`load_meta_arch`, `build_reference_model`, `to_d2_inputs`) with the reference class in place of WeaklySupervisedRCNNNoMeta.

Inputs are NOT stored: `pseudo_inputs()` below regenerates them from seeds at the tiny shapes of gen_ref_step.py (R50, 96x128, 300 -> 50
proposals, K = 20, two Res5 heads, 2 supervised + 2 weak images) -- the tests call the same function. Recorded per case ("on" / "off" =
MODEL.ROI_HEADS.TRAIN_PROPOSAL_REGRESSOR): the loss dictionary, the weak images' eval-mode detections, the reference's pseudo ground truth
and the detection rows it kept, the weak anchor labels, each weak image's own RPN losses, and gradient norms / heads of
proposal_generator.rpn_head.* and of gen_unit_golden.GRAD_KEYS.

The threshold is MEASURED: synthetic weights do not score 0.99, so a first reference run with threshold 0 yields the detections' scores
and the threshold becomes the midpoint between two neighbouring scores of label-matching detections such that one weak image keeps >= 2
pseudo ground-truth boxes and the other none. The conditions that make the fixture meaningful are asserted (`check_conditions`, shared with
tests/test_rpn_pseudo_cpu.py). Only numeric arrays go into the .npz.   Run here:  python tests/golden/gen_rpn_pseudo_golden.py

ONE STATEMENT PAIR OF THE REFERENCE IS STEPPED OVER. As written, the class cannot run a weak batch with TRAIN_USING_WEAK off (its default):
the `else:` of rcnn.py:618-620 -- the branch taken whenever TRAIN_USING_WEAK is off -- appends to two dictionary keys that exist only when
the switch is on (:589-591) and reads a variable only the other branch assigns (:586), so the forward raises KeyError at :619. Those two
statements feed `weak_loss_cls` / `weak_loss_bbox`, losses of the TRAIN_USING_WEAK branch alone; nothing this fixture records depends on
them. `load_meta_arch_runnable` compiles the file with lines 619-620 blanked to `pass` (addressed by line number and checked by a hash, so
no reference text is held here) and every other line as it is: the backbone / RPN / eval ROI heads / selection / per-image RPN loss /
combination arithmetic of :550-609 and :622-654 is the reference's own.
"""
import hashlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p_ in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

OUT = os.path.join(HERE, "rpn_pseudo_golden.npz")
CASES = ("on", "off")
WEIGHT_SEED, DATA_SEED, PERM_SEED = 11, 368, 57
DIVISOR = 1.0
# every label-matching score must be further than this (relative) from the threshold: bf16 activations move a score by up to ~2^-8
# relative per rounding; the bf16 step must reproduce the fp32 step's kept rows
BF16_MARGIN = 0.02


def pseudo_inputs(device="cpu", regressor=True, threshold=None):
    """-> (cfg, model, sup, weak, perms). Deterministic; shared by the generator and the tests. threshold None: the fixture's."""
    import gen_ref_step as S
    from unit_amd.modeling import build_model
    from unit_amd.synthetic import init_synthetic_weights, synthetic_batch
    if threshold is None:
        threshold = float(np.load(OUT)["threshold"])
    cfg = S.case_cfg("s1", device)
    cfg.MODEL.META_ARCHITECTURE = "WeaklySupervisedRCNNRPN"
    cfg.MODEL.PROPOSAL_GENERATOR.WEAK_RPN_SCORE_TRESHOLD = float(threshold)
    cfg.MODEL.ROI_HEADS.TRAIN_PROPOSAL_REGRESSOR = bool(regressor)
    cfg.MODEL.ROI_HEADS.WEAK_PROPOSAL_DIVISOR = DIVISOR
    K = cfg.MODEL.ROI_HEADS.NUM_CLASSES
    model = build_model(cfg)
    init_synthetic_weights(model, seed=WEIGHT_SEED)
    g = torch.Generator().manual_seed(PERM_SEED)
    with torch.no_grad():
        bp = model.roi_heads.box_predictor
        bp.cls_score_delta.weight.copy_(torch.randn(bp.cls_score_delta.weight.shape, generator=g) * 0.02)
    from unit_amd.layers import invalidate_prepared
    invalidate_prepared()
    sup, weak = synthetic_batch(2, 2, hw=S.HW, num_classes=K, base_ids=list(cfg.DATASETS.FEWSHOT.BASE_CLASSES_ID), seed=DATA_SEED, max_gt=3)
    n_anchor = (S.HW[0] // 16) * (S.HW[1] // 16) * 15
    perms = dict(rpn=[torch.randperm(n_anchor, generator=g) for _ in sup], roi=[torch.randperm(50 + 3, generator=g) for _ in sup],
                 weak_rpn=[torch.randperm(n_anchor, generator=g) for _ in weak])
    return cfg, model, sup, weak, perms


def select(scores, classes, labels, threshold):
    """rcnn.py:594-597 restated: rows whose class is one of `labels` and whose score is strictly above the threshold, in order"""
    scores, classes = np.asarray(scores), np.asarray(classes)
    keep = np.isin(classes, np.asarray(labels)) & (scores > np.float32(threshold))
    return np.nonzero(keep)[0]


def check_conditions(fx):
    """what makes the fixture meaningful (ISSUE): one weak image keeps >= 2 pseudo GT, the other none; a detection is dropped by label and
    one by score; both weak losses are non-zero in the "on" case; every label-matching score keeps BF16_MARGIN from the threshold"""
    thr = float(fx["threshold"])
    kept = [len(fx[f"on/weak/kept{i}"]) for i in range(2)]
    assert max(kept) >= 2 and min(kept) == 0, kept
    by_label = by_score = 0
    for i in range(2):
        sc, cl, lab = fx[f"on/weak/det_scores{i}"], fx[f"on/weak/det_classes{i}"], fx[f"on/weak/labels{i}"]
        m = np.isin(cl, lab)
        by_label += int((~m).sum())
        by_score += int((m & ~(sc > np.float32(thr))).sum())
        assert (np.abs(sc[m] - thr) > BF16_MARGIN * thr).all(), (sc[m], thr)
    assert by_label >= 1 and by_score >= 1, (by_label, by_score)
    names = [str(n) for n in fx["on/loss_names"]]
    for k in ("weak_loss_rpn_cls", "weak_loss_rpn_loc"):
        assert fx["on/losses"][names.index(k)] != 0.0, k
    assert fx["off/losses"][[str(n) for n in fx["off/loss_names"]].index("weak_loss_rpn_loc")] == 0.0


def run_reference(G, regressor, threshold):
    """one training forward + backward of the reference class -> (losses, trace, p, model)"""
    import gen_ref_step as S
    orc = sys.modules["unit_oracle"]
    cfg, model, sup, weak, perms = pseudo_inputs(regressor=regressor, threshold=threshold)
    p = S.oracle_params(model)
    ocfg = S.oracle_cfg(cfg)
    MA = G.REF["meta"]
    plain = MA.WeaklySupervisedRCNNNoMeta
    MA.WeaklySupervisedRCNNNoMeta = lambda **kw: MA.WeaklySupervisedRCNNRPN(
        weak_rpn_score_threshold=threshold, train_using_weak=False, train_proposal_regressor=regressor, weak_proposal_divisor=DIVISOR, **kw)
    try:
        ref, trace = G.build_reference_model(p, ocfg, perms, roi_cls=cfg.MODEL.ROI_HEADS.NAME, pred_cls=cfg.MODEL.ROI_HEADS.FAST_RCNN.NAME)
    finally:
        MA.WeaklySupervisedRCNNNoMeta = plain
    assert type(ref).__name__ == "WeaklySupervisedRCNNRPN"
    ref.roi_heads.visual_threshold = ocfg["visual_threshold"]
    ref.roi_heads.box_predictor._freeze_layers(list(cfg.MODEL.FREEZE_LAYERS.FAST_RCNN))
    rpn, heads = ref.proposal_generator, ref.roi_heads
    trace["weak_anchor_labels"], trace["weak_image_losses"] = {}, {}

    heads_forward = heads.forward

    def forward(*a, **k):          # the eval-mode call of rcnn.py:578: note the detections down, number their rows
        out = heads_forward(*a, **k)
        if not heads.training:
            for inst in out[0]:
                inst.det_index = torch.arange(len(inst))
            trace["weak_det"] = [(i.pred_boxes.tensor.clone(), i.scores.clone(), i.pred_classes.clone()) for i in out[0]]
            trace["weak_pred"] = out[0]          # the list the reference filters in place (:595-599)
        return out
    heads.forward = forward

    def label_and_sample_anchors(anchors, gt_instances):
        if gt_instances[0].has("pred_boxes"):          # rcnn.py:601: one weak image with its pseudo ground truth
            idx, = [i for i, w in enumerate(trace["weak_pred"]) if w is gt_instances[0]]
            gl, gb = orc.label_and_sample_anchors(anchors[0].tensor, [gt_instances[0].gt_boxes.tensor], [perms["weak_rpn"][idx]])
            trace["weak_anchor_labels"][idx] = gl[0]
            trace["cur_weak"] = idx
            return gl, gb
        gl, gb = orc.label_and_sample_anchors(anchors[0].tensor, [g.gt_boxes.tensor for g in gt_instances], perms["rpn"])
        trace["anchor_labels"] = gl
        return gl, gb
    rpn.label_and_sample_anchors = label_and_sample_anchors
    rpn_losses = rpn.losses

    def losses_spy(*a, **k):
        out = rpn_losses(*a, **k)
        if trace.get("cur_weak") is not None:
            trace["weak_image_losses"][trace.pop("cur_weak")] = {n: v.item() for n, v in out.items()}
        return out
    rpn.losses = losses_spy
    ref.train()
    losses = ref(G.to_d2_inputs(sup), G.to_d2_inputs(weak))
    sum(losses.values()).backward()
    trace["weak_labels"] = [x["instances"].gt_classes for x in weak]
    return losses, trace, p, ref


def measure_threshold(G):
    """the threshold from the reference run's own scores: the weak image with the best second label-matching score keeps its top two, the other
    image none -- the midpoint between that second score and the next label-matching score below it (of either image)"""
    _, trace, _, _ = run_reference(G, True, 0.0)
    match = []
    for (_, sc, cl), lab in zip(trace["weak_det"], trace["weak_labels"]):
        m = (cl.unsqueeze(1) == lab.unsqueeze(0)).any(1)
        match.append(sc[m].sort(descending=True).values)
        print("weak image:", len(sc), "detections,", int(m.sum()), "of its labels", lab.tolist(), "scores", [round(v, 4) for v in match[-1].tolist()[:6]])
    a = max(range(2), key=lambda i: match[i][1].item() if len(match[i]) > 1 else -1.0)
    assert len(match[a]) > 1, "no weak image has two label-matching detections: change the seeds"
    second = match[a][1].item()
    below = torch.cat(match)
    below = below[below < second]
    assert len(below) > 0, "no label-matching detection below the chosen pair: change the seeds"
    nxt = below.max().item()
    assert len(match[1 - a]) == 0 or match[1 - a][0].item() <= nxt, "the other weak image would keep a detection too: change the seeds"
    return 0.5 * (second + nxt)


REF_RCNN = "/root/reference/modeling/meta_arch/rcnn.py"
DEAD_ELSE_SHA256 = "c46e52ee6b34402ae747ee19c6f153d6be23e67ed277a003ea72004eed92cdc9"          # of lines 618-620 as they stand in the reference


def load_meta_arch_runnable(G):
    """G.load_meta_arch() (the Detectron2 stand-ins the file imports), then the same file once more with the two statements of its `else:` at
    :619-620 replaced by `pass` (module docstring): line numbers unchanged, nothing else touched"""
    G.load_meta_arch()
    lines = open(REF_RCNN).read().split("\n")
    assert hashlib.sha256("\n".join(lines[617:620]).encode()).hexdigest() == DEAD_ELSE_SHA256, "the reference changed: re-read rcnn.py:611-620"
    indent = len(lines[618]) - len(lines[618].lstrip())
    lines[618], lines[619] = " " * indent + "pass", ""
    m = types.ModuleType("ref_unit.modeling.meta_arch.rcnn_runnable")
    m.__file__ = REF_RCNN
    exec(compile("\n".join(lines), REF_RCNN, "exec"), m.__dict__)
    G.REF["meta"] = m


def main(out_path=None):
    import gen_unit_golden as G
    load_meta_arch_runnable(G)
    thr = measure_threshold(G)
    out = {"threshold": np.array(thr, dtype=np.float64), "divisor": np.array(DIVISOR)}
    for tag, reg in (("on", True), ("off", False)):
        losses, trace, p, ref = run_reference(G, reg, thr)
        G.collect_step(out, tag, ref, losses, trace, p)
        for k in sorted(p):
            if k.startswith("proposal_generator.rpn_head.") and p[k].grad is not None:
                out[f"{tag}/gradnorm/{k}"] = np.array(p[k].grad.double().norm().item())
                out[f"{tag}/gradhead/{k}"] = G.npy(p[k].grad.reshape(-1)[:256])
        for i, ((b, sc, cl), lab) in enumerate(zip(trace["weak_det"], trace["weak_labels"])):
            out[f"{tag}/weak/det_boxes{i}"], out[f"{tag}/weak/det_scores{i}"], out[f"{tag}/weak/det_classes{i}"] = G.npy(b), G.npy(sc), G.npy(cl)
            out[f"{tag}/weak/labels{i}"] = G.npy(lab)
            kept = trace["weak_pred"][i]          # what the reference's own two masks left (:595, :597)
            out[f"{tag}/weak/kept{i}"], out[f"{tag}/weak/pseudo_boxes{i}"] = G.npy(kept.det_index), G.npy(kept.gt_boxes.tensor)
            if i in trace["weak_anchor_labels"]:
                out[f"{tag}/weak/anchor_labels{i}"] = G.npy(trace["weak_anchor_labels"][i]).astype(np.int8)
                il = trace["weak_image_losses"][i]
                out[f"{tag}/weak/image_losses{i}"] = np.array([il["loss_rpn_cls"], il["loss_rpn_loc"]], dtype=np.float64)
        print(tag, {k: round(v.item(), 6) for k, v in sorted(losses.items())}, "kept", [len(trace["weak_pred"][i]) for i in range(2)])
    check_conditions(out)
    np.savez_compressed(out_path or OUT, **out)
    print("wrote", out_path or OUT, len(out), "arrays", os.path.getsize(out_path or OUT), "bytes; threshold", thr)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
