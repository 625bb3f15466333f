"""Generates tests/golden/only_weak_golden.npz by RUNNING THE REFERENCE'S OWN weak-only training mode in the authoring container:
`WeaklySupervisedRCNNNoMeta.forward(None, weak_batched_inputs=W, train_only_weak=True)` (/root/reference/modeling/meta_arch/rcnn.py:433-491,
the step of TrainerOnlyWeak, engine/defaults.py:377-400) on the stubbed Detectron2 modules of gen_unit_golden.py (`load_meta_arch`,
`build_reference_model`, `to_d2_inputs`), for THREE iterations of the reference's solver/build.py:build_optimizer_C4 -> torch.optim.SGD with
d2's WarmupMultiStepLR (zero_grad -> backward -> step -> scheduler, as gen_ref_step.trajectory does for the default step).

Inputs are NOT stored: `only_weak_inputs(case)` below regenerates them from seeds at the tiny shapes of gen_ref_step.py (R50, 96x128,
300 -> 50 proposals, K = 20, 2 weak images) -- the tests call the same function. No input is a random permutation: the weak half samples
nothing, and the generator asserts that the reference draws none. Cases: "ow" (two Res5 heads, TYPE "OICR"), "ow_single" (MULTI_BOX_HEAD
False), "ow_reg" (WEAK_DETECTOR.REGRESSION_BRANCH, FINETUNE_TERMS ["lingual"]).

Recorded per iteration: the loss dictionary (keys too), gradient norms / heads of gen_unit_golden.GRAD_KEYS and of the predictors' tensors.
Once: the names of the trainable parameters whose .grad is None (the same set on every iteration: asserted). After the last iteration: a
strided sample of every trainable tensor and whether it still equals its initial bits. `check_conditions` (shared with
tests/test_only_weak_cpu.py) asserts what makes the fixture meaningful. Only numeric / name arrays go into the .npz.
Run here:  python tests/golden/gen_only_weak_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p_ in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

OUT = os.path.join(HERE, "only_weak_golden.npz")
CASES = ("ow", "ow_single", "ow_reg")
STEPS = 3
WEIGHT_SEED, DATA_SEED, DELTA_SEED = 23, 415, 61
SAMPLE = 256


def only_weak_cfg(case, device="cpu"):
    """gen_ref_step's "s1" configuration and trajectory solver (non-trivial per-name factors, two warm-up iterations), the step decay moved
    to iteration 2 so that three iterations see warm-up, the base rate times gamma and every parameter group"""
    import gen_ref_step as S
    c = S.traj_cfg(device, "s1")
    c.SOLVER.STEPS = (2,)
    if case == "ow_single":
        c.MODEL.ROI_HEADS.MULTI_BOX_HEAD = False
    if case == "ow_reg":
        c.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR.REGRESSION_BRANCH = True
        ft = c.MODEL.ROI_HEADS.FINETUNE_TERMS
        ft.CLASSIFIER, ft.BBOX, ft.MASK = ["lingual"], ["lingual"], ["lingual"]
    return c


def only_weak_inputs(case, device="cpu"):
    """-> (cfg, model, weak). Deterministic; shared by the generator and the tests."""
    import gen_ref_step as S
    from unit_amd.layers import invalidate_prepared
    from unit_amd.modeling import build_model
    from unit_amd.synthetic import init_synthetic_weights, synthetic_batch
    cfg = only_weak_cfg(case, device)
    K = cfg.MODEL.ROI_HEADS.NUM_CLASSES
    model = build_model(cfg)
    init_synthetic_weights(model, seed=WEIGHT_SEED + CASES.index(case))
    g = torch.Generator().manual_seed(DELTA_SEED)
    with torch.no_grad():
        bp = model.roi_heads.box_predictor
        bp.cls_score_delta.weight.copy_(torch.randn(bp.cls_score_delta.weight.shape, generator=g) * 0.02)
    invalidate_prepared()
    _, weak = synthetic_batch(1, 2, hw=S.HW, num_classes=K, base_ids=list(cfg.DATASETS.FEWSHOT.BASE_CLASSES_ID),
                              seed=DATA_SEED + CASES.index(case), max_gt=3)
    return cfg, model, weak


def sample(t):
    """the elements of a parameter tensor the fixture keeps: every stride-th, at most SAMPLE"""
    f = t.detach().reshape(-1)
    return f[::max(1, f.numel() // SAMPLE)][:SAMPLE]


def group_of(name):
    """which part of the model a trainable tensor belongs to (check_conditions)"""
    if name.startswith("backbone."):
        return "backbone"
    if ".res5." in name:
        return "res5"
    if ".weak_detector_head." in name:
        return "weak_predictor"
    return "other"


def check_conditions(fx):
    """what makes the fixture meaningful (ISSUE): every dead tensor kept its initial bits; a live tensor of each of backbone, Res5 head and
    weak predictor moved; the dead set holds the RPN head and the delta predictors, with two Res5 heads also box_head; the loss keys are
    the reference's of this mode"""
    for case in CASES:
        names = [str(n) for n in fx[f"{case}/names"]]
        dead = {str(n) for n in fx[f"{case}/dead_names"]}
        unchanged = dict(zip(names, fx[f"{case}/unchanged"].tolist()))
        assert dead <= set(names) and dead, case
        assert all(unchanged[n] for n in dead), [n for n in dead if not unchanged[n]]
        moved = {group_of(n) for n in names if n not in dead and not unchanged[n]}
        assert {"backbone", "res5", "weak_predictor"} <= moved, (case, moved)
        assert any(n.startswith("proposal_generator.rpn_head.") for n in dead), case
        for d in ("cls_score_delta", "bbox_pred_delta"):
            assert f"roi_heads.box_predictor.{d}.weight" in dead and f"roi_heads.box_predictor.{d}.bias" in dead, (case, d)
        has_box_head = any(n.startswith("roi_heads.box_head.") for n in dead)
        assert has_box_head == (case != "ow_single"), case
        assert not any(n.startswith("roi_heads.weak_box_head.") or ".weak_detector_head." in n or n.startswith("backbone.") for n in dead), case
        keys = ["loss_im_cls", "loss_oicr_1", "loss_oicr_2", "loss_oicr_3"] + \
               (["loss_regression_bbox", "loss_regression_cls"] if case == "ow_reg" else [])
        assert [str(n) for n in fx[f"{case}/loss_names"]] == sorted(keys), (case, fx[f"{case}/loss_names"])
        assert fx[f"{case}/losses"].shape == (STEPS, len(keys)) and np.isfinite(fx[f"{case}/losses"]).all()
        assert int(fx[f"{case}/permutations_drawn"]) == 0, case


def regression_weak_head(G, pred, p, K):
    """the reference's WeakDetectorOutputsBase with its regression branch, holding the model's weights (build_reference_model builds the
    head without the branch)"""
    d2, REF = G.d2, G.REF
    pre = "roi_heads.box_predictor.weak_detector_head."
    old = pred.weak_detector_head
    head = REF["weak"].WeakDetectorOutputsBase(
        d2.ShapeSpec(channels=p[pre + "classifier_stream.weight"].shape[1]), box2box_transform=d2.Box2BoxTransform((10.0, 10.0, 5.0, 5.0)),
        num_classes=K, oicr_iter=3, fg_threshold=0.5, bg_threshold=0.1, mil_multiplier=old.mil_multiplier, detector_temp=old.detector_temp,
        classifier_temp=old.classifier_temp, weak_detector_type="OICR", regression_branch=True, smooth_l1_beta=0.0, box_reg_loss_type="smooth_l1",
        proposal_matcher=REF["matcher"].Matcher([0.5], [0, 1], allow_low_quality_matches=False), test_score_thresh=0.05,
        base_classes=old.base_classes, novel_classes=old.novel_classes)
    head.load_state_dict({k[len(pre):]: v.detach().clone() for k, v in p.items() if k.startswith(pre)})
    return head


def run_reference(G, case, out):
    from torch import nn
    import gen_ref_step as S
    d2 = G.d2
    cfg, model, weak = only_weak_inputs(case)
    p = S.oracle_params(model)
    ocfg = S.oracle_cfg(cfg)
    # (build_reference_model builds the weak head without the regression branch: its four tensors step aside while it loads the others)
    aside = {k: p.pop(k) for k in [k for k in p if ".regression_branch_" in k]}
    ref, trace = G.build_reference_model(p, ocfg, None, roi_cls=cfg.MODEL.ROI_HEADS.NAME, pred_cls=cfg.MODEL.ROI_HEADS.FAST_RCNN.NAME)
    p.update(aside)
    ref.roi_heads.visual_threshold = ocfg["visual_threshold"]
    pred = ref.roi_heads.box_predictor
    if case == "ow_reg":
        if not hasattr(d2.FastRCNNOutputs, "_predict_boxes"):          # Detectron2 v0.3 (gen_regression_branch_golden.py)
            d2.FastRCNNOutputs._predict_boxes = lambda self: self.box2box_transform.apply_deltas(self.pred_proposal_deltas, self.proposals.tensor)
        pred.weak_detector_head = regression_weak_head(G, pred, p, ocfg["num_classes"])
        pred.regression_branch = True
    pred._freeze_layers(list(cfg.MODEL.FREEZE_LAYERS.FAST_RCNN))
    # every TRAINABLE tensor of the d2-ext blocks into the module tree under its Detectron2 name (gen_ref_step.trajectory)
    pred_prefix = "roi_heads.box_predictor."
    for k in sorted(p):
        if not p[k].requires_grad or k.startswith(pred_prefix):
            continue
        parts, mod = k.split("."), ref
        for a in parts[:-1]:
            if a not in mod._modules:
                mod.add_module(a, nn.Module())
            mod = mod._modules[a]
        par = nn.Parameter(p[k].detach().clone())
        mod.register_parameter(parts[-1], par)
        p[k] = par
    named = {pred_prefix + n_: q for n_, q in pred.named_parameters() if q.requires_grad}
    named.update({k: v for k, v in p.items() if isinstance(v, nn.Parameter)})
    want = {n_ for n_, q in model.named_parameters() if q.requires_grad}
    assert set(named) == want, sorted(set(named) ^ want)[:8]
    for k, q in named.items():          # the reference head holds the model's values
        assert torch.equal(q.detach(), model.state_dict()[k]), k
    start = {k: v.detach().clone() for k, v in named.items()}
    opt = G.d2.load_reference_solver().build_optimizer_C4(cfg, ref)
    assert sum(len(g["params"]) for g in opt.param_groups) == len(named)
    sched = G.d2.WarmupMultiStepLR(opt, cfg.SOLVER.STEPS, cfg.SOLVER.GAMMA, warmup_factor=cfg.SOLVER.WARMUP_FACTOR,
                                   warmup_iters=cfg.SOLVER.WARMUP_ITERS)
    ref.train()
    d2_weak = G.to_d2_inputs(weak)
    drawn = [0]
    randperm = torch.randperm

    def counting_randperm(*a, **k):
        drawn[0] += 1
        return randperm(*a, **k)
    torch.randperm = counting_randperm
    dead0, losses_all = None, []
    try:
        for it in range(STEPS):
            losses = ref(None, weak_batched_inputs=d2_weak, train_only_weak=True)          # engine/defaults.py:391
            opt.zero_grad()
            sum(losses.values()).backward()
            dead = sorted(k for k, q in named.items() if q.grad is None)
            assert dead0 is None or dead == dead0
            dead0 = dead
            G.collect_step(out, f"{case}/it{it}", ref, losses, trace, p)
            opt.step()
            sched.step()
            losses_all.append([losses[k].item() for k in sorted(losses)])
            print(case, it, {k: round(v.item(), 6) for k, v in sorted(losses.items())})
    finally:
        torch.randperm = randperm
    assert "sampled" not in trace and "anchor_labels" not in trace          # neither sampler ran
    out[f"{case}/permutations_drawn"] = np.array(drawn[0])
    out[f"{case}/loss_names"] = np.array(sorted(losses))
    out[f"{case}/losses"] = np.array(losses_all, dtype=np.float64)
    names = sorted(named)
    out[f"{case}/names"] = np.array(names)
    out[f"{case}/dead_names"] = np.array(dead0)
    out[f"{case}/unchanged"] = np.array([bool(torch.equal(named[k].detach(), start[k])) for k in names], dtype=np.uint8)
    for k in names:
        out[f"{case}/final_sample/{k}"] = G.npy(sample(named[k]))


def main(out_path=None):
    import gen_unit_golden as G
    G.load_meta_arch()
    out = {}
    for case in CASES:
        run_reference(G, case, out)
    check_conditions(out)
    np.savez_compressed(out_path or OUT, **out)
    print("wrote", out_path or OUT, len(out), "arrays", os.path.getsize(out_path or OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
