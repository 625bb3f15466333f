"""Generates tests/golden/load_proposals_golden.npz by RUNNING THE REFERENCE'S OWN WSROIHeadNoMeta training forward with
`load_proposals = True` (modeling/roi_heads/roi_heads.py:553-584: the weak images' proposals are not cut to their first
BATCH_SIZE_PER_IMAGE // WEAK_CLASSIFIER_PROPOSAL_DIVISOR rows), inside the reference's WeaklySupervisedRCNNNoMeta.forward
(meta_arch/rcnn.py:433-491) on the stubbed Detectron2 modules of gen_unit_golden.py (`load_meta_arch`, `build_reference_model`,
`to_d2_inputs`). The reference's text is imported by file and not touched; only numbers and names go into the .npz.

The model is gen_ref_step.py's reduced one (R50, 96 x 128 images, 16 sampled RoIs per supervised image, K = 20, two supervised and two weak
images). The RPN call for the WEAK images (rcnn.py:468-470, under no_grad) is answered with GIVEN proposals -- 1100 for the first weak image,
1500 for the second, so that the second is ragged against the first -- which is what a dataset with precomputed proposals hands the model
there; the supervised images keep the proposals the reference's RPN makes (50 each), and these are recorded, because a device RPN decodes
them with other last bits. Cases: "lp_oicr" (TYPE "OICR"), "lp_reg" (OICR with WEAK_DETECTOR.REGRESSION_BRANCH) and "lp_pcl" (TYPE "PCL",
under the stable argsort that is this project's canonical tie rule, as gen_regression_branch_golden.py runs it).

Not stored, regenerated from seeds by `lp_inputs(case)` (the tests call it too): weights, images, labels, sampling permutations.
Stored: the weak proposals (one set for all cases), the supervised proposals, every loss of the step, and for the OICR cases the labels and
weights of every compute_loss_inputs call (weak_detector_fast_rcnn.py:378-408: iterations 0..2, then the regression branch's), row by row
in the order of the proposals.

Conditions the generator asserts (a seed that fails is replaced, `--search`): the weak head's losses are evaluated again on its own
recorded logits under four relative perturbations of 2^-18 (an fp32 network on other hardware reproduces logits to ~2^-20): no OICR label
moves, no weight moves by more than 1e-4 of the largest, no loss by more than 2e-5 relative -- so a 1e-4 comparison of losses and an exact
comparison of labels are meaningful; each weak image has rows above FG_THRESHOLD, between the thresholds and under BG_THRESHOLD.
Run here:  python tests/golden/gen_load_proposals_golden.py [output path]"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p_ in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

OUT = os.path.join(HERE, "load_proposals_golden.npz")
# case -> (WEAK_DETECTOR.TYPE, REGRESSION_BRANCH)
CASES = {"lp_oicr": ("OICR", False), "lp_reg": ("OICR", True), "lp_pcl": ("PCL", False)}
WEAK_SIZES = (1100, 1500)
WEIGHT_SEED, DATA_SEED, DELTA_SEED, BOX_SEED = 31, 523, 67, 811
PERTURBATIONS, EPS = 4, 2.0 ** -18
_ARGSORT = torch.Tensor.argsort


def _stable_argsort(self, dim=-1, descending=False, stable=True):
    return torch.sort(self, dim=dim, descending=descending, stable=True)[1]


def lp_cfg(case, device="cpu"):
    """gen_ref_step's "s1" configuration with MODEL.LOAD_PROPOSALS on and the case's weak detector"""
    import gen_ref_step as S
    typ, reg = CASES[case]
    c = S.case_cfg("s1", device)
    c.MODEL.LOAD_PROPOSALS = True
    wd = c.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR
    wd.TYPE, wd.REGRESSION_BRANCH = typ, reg
    if reg:          # (the branch with the shipped "lingual" terms, as gen_only_weak_golden.py's "ow_reg")
        ft = c.MODEL.ROI_HEADS.FINETUNE_TERMS
        ft.CLASSIFIER, ft.BBOX, ft.MASK = ["lingual"], ["lingual"], ["lingual"]
    return c


def lp_inputs(case, device="cpu"):
    """-> (cfg, model, sup, weak, perms). Deterministic; shared by the generator and the tests."""
    import gen_ref_step as S
    from unit_amd.layers import invalidate_prepared
    from unit_amd.modeling import build_model
    from unit_amd.synthetic import init_synthetic_weights, synthetic_batch
    cfg = lp_cfg(case, device)
    K = cfg.MODEL.ROI_HEADS.NUM_CLASSES
    model = build_model(cfg)
    init_synthetic_weights(model, seed=WEIGHT_SEED)
    g = torch.Generator().manual_seed(DELTA_SEED)
    with torch.no_grad():
        bp = model.roi_heads.box_predictor
        bp.cls_score_delta.weight.copy_(torch.randn(bp.cls_score_delta.weight.shape, generator=g) * 0.02)
    invalidate_prepared()
    sup, weak = synthetic_batch(2, 2, hw=S.HW, num_classes=K, base_ids=list(cfg.DATASETS.FEWSHOT.BASE_CLASSES_ID), seed=DATA_SEED, max_gt=3)
    n_anchor = (S.HW[0] // 16) * (S.HW[1] // 16) * 15
    perms = dict(rpn=[torch.randperm(n_anchor, generator=g) for _ in sup],
                 roi=[torch.randperm(cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN + 3, generator=g) for _ in sup])
    return cfg, model, sup, weak, perms


def weak_boxes(seed=BOX_SEED, hw=(96, 128)):
    """the given proposals of the two weak images: two thirds scattered around three centres (every IoU band occurs, many near-duplicates),
    one third anywhere in the image; fp32, inside the image, at least 6 px a side"""
    g = torch.Generator().manual_seed(seed)
    h, w = float(hw[0]), float(hw[1])
    centers = torch.tensor([[34.0, 30.0, 40.0, 36.0], [90.0, 58.0, 48.0, 44.0], [64.0, 44.0, 22.0, 60.0]])
    out = []
    for n in WEAK_SIZES:
        c = centers[torch.randint(0, len(centers), (n,), generator=g)]
        jit = (torch.rand(n, 4, generator=g) - 0.5) * torch.tensor([14.0, 14.0, 28.0, 28.0])
        cx, cy, bw, bh = c[:, 0] + jit[:, 0], c[:, 1] + jit[:, 1], (c[:, 2] + jit[:, 2]).clamp(min=6), (c[:, 3] + jit[:, 3]).clamp(min=6)
        anywhere = torch.rand(n, generator=g) < 1.0 / 3
        u = torch.rand(n, 4, generator=g)
        cx, cy = torch.where(anywhere, u[:, 0] * w, cx), torch.where(anywhere, u[:, 1] * h, cy)
        bw, bh = torch.where(anywhere, 6 + u[:, 2] * 70, bw), torch.where(anywhere, 6 + u[:, 3] * 60, bh)
        b = torch.stack([(cx - bw / 2).clamp(0, w - 6), (cy - bh / 2).clamp(0, h - 6), (cx + bw / 2).clamp(6, w), (cy + bh / 2).clamp(6, h)], 1)
        b[:, 2] = torch.maximum(b[:, 2], b[:, 0] + 6)
        b[:, 3] = torch.maximum(b[:, 3], b[:, 1] + 6)
        out.append(b.contiguous())
    return out


def npy(t):
    a = t.detach().cpu().numpy()
    return a.astype(np.int32) if a.dtype.kind in "iu" else a.astype(np.float32)


def run_reference(G, case, boxes):
    """-> dict(losses, sup_props, calls [(labels, weights)], why): one training forward of the reference on the case"""
    import gen_ref_step as S
    import unit_oracle as orc
    d2 = G.d2
    typ, reg = CASES[case]
    cfg, model, sup, weak, perms = lp_inputs(case)
    p = S.oracle_params(model)
    ocfg = S.oracle_cfg(cfg)
    aside = {k: p.pop(k) for k in [k for k in p if ".regression_branch_" in k]}
    ref, trace = G.build_reference_model(p, ocfg, perms, roi_cls=cfg.MODEL.ROI_HEADS.NAME, pred_cls=cfg.MODEL.ROI_HEADS.FAST_RCNN.NAME)
    p.update(aside)
    ref.roi_heads.visual_threshold = ocfg["visual_threshold"]
    ref.roi_heads.load_proposals = True                                  # roi_heads.py:184: cfg.MODEL.LOAD_PROPOSALS
    pred = ref.roi_heads.box_predictor
    if reg:
        import gen_only_weak_golden as OW
        if not hasattr(d2.FastRCNNOutputs, "_predict_boxes"):          # Detectron2 v0.3 (gen_regression_branch_golden.py)
            d2.FastRCNNOutputs._predict_boxes = lambda self: self.box2box_transform.apply_deltas(self.pred_proposal_deltas, self.proposals.tensor)
        pred.weak_detector_head = OW.regression_weak_head(G, pred, p, ocfg["num_classes"])
        pred.regression_branch = True
    head = pred.weak_detector_head
    head.weak_detector_type = typ
    pred._freeze_layers(list(cfg.MODEL.FREEZE_LAYERS.FAST_RCNN))
    # the RPN's second call of the step is the weak images' (rcnn.py:468-470): answered with the given proposals
    find, calls = orc.find_top_rpn_proposals, [0]

    def given(*a, **k):
        calls[0] += 1
        return [(b.clone(), torch.zeros(len(b))) for b in boxes] if calls[0] == 2 else find(*a, **k)
    orc.find_top_rpn_proposals = given
    rec, seen = [], {}
    orig_inputs, orig_losses = head.compute_loss_inputs, head.losses

    def spy_inputs(*a, **k):
        r = orig_inputs(*a, **k)
        lab = torch.cat([q.gt_classes for q in r["proposals"]]) if "proposals" in r else r["labels"]
        rec.append((lab.clone(), r["cls_weights"].clone()))
        return r

    def spy_losses(weak_predictions, weak_proposals, weak_targets):
        seen.update(preds=weak_predictions, props=weak_proposals, targets=weak_targets)
        return orig_losses(weak_predictions, weak_proposals, weak_targets)
    head.compute_loss_inputs, head.losses = spy_inputs, spy_losses
    torch.Tensor.argsort = _stable_argsort if typ == "PCL" else _ARGSORT
    ref.train()
    try:
        with torch.no_grad():
            losses = ref(G.to_d2_inputs(sup), G.to_d2_inputs(weak))
        assert calls[0] == 2 and [len(q) for q in seen["props"]] == list(WEAK_SIZES), "the reference cut the weak proposals"
        first = list(rec)
        base = {k: float(v) for k, v in orig_losses(seen["preds"], seen["props"], seen["targets"]).items()}
        del rec[len(first):]
        why = None
        gp = torch.Generator().manual_seed(BOX_SEED + 7)
        for _ in range(PERTURBATIONS):
            def shake(t):
                if t is None or isinstance(t, list):
                    return [shake(x) for x in t] if isinstance(t, list) else None
                return t.detach() * (1 + (torch.rand(t.shape, generator=gp) * 2 - 1) * EPS)
            n0 = len(rec)
            moved = orig_losses([shake(t) for t in seen["preds"]], seen["props"], seen["targets"])
            for (la, wa), (lb, wb) in zip(first, rec[n0:]):
                if not torch.equal(la, lb):
                    why = why or f"{int((la != lb).sum())} OICR labels move under a 2^-18 perturbation"
                elif float((wa - wb).abs().max()) > 1e-4 * float(wa.abs().max()):
                    why = why or "an OICR weight moves under a 2^-18 perturbation"
            for k, v in moved.items():
                if not abs(float(v) - base[k]) <= 2e-5 * max(1.0, abs(base[k])):
                    why = why or f"{k} moves from {base[k]} to {float(v)} under a 2^-18 perturbation"
            del rec[n0:]
    finally:
        torch.Tensor.argsort = _ARGSORT
        orc.find_top_rpn_proposals = find
    if why is None and typ == "OICR":
        K, idx = ocfg["num_classes"], np.insert(np.cumsum(WEAK_SIZES), 0, 0)
        for lab, w in first:
            for i in range(2):
                l_, w_ = lab[idx[i]:idx[i + 1]], w[idx[i]:idx[i + 1]]
                if not (bool((l_ < K).any()) and bool(((l_ == K) & (w_ > 0)).any()) and bool((w_ == 0).any())):
                    why = why or f"weak image {i}: not every IoU band occurs"
    return dict(losses=losses, sup_props=trace["proposals"][0], calls=first, why=why, base=base)


def main(out_path=None, search=False):
    import gen_unit_golden as G
    G.load_meta_arch()
    seed = BOX_SEED
    while True:
        boxes = weak_boxes(seed)
        runs = {case: run_reference(G, case, boxes) for case in CASES}
        bad = {c: r["why"] for c, r in runs.items() if r["why"]}
        print("box seed", seed, bad or "ok", flush=True)
        if not bad:
            break
        assert search, f"BOX_SEED {seed}: {bad} -- reseed (python gen_load_proposals_golden.py --search)"
        seed += 1
    assert seed == BOX_SEED, f"commit BOX_SEED = {seed}"
    out = {"cases": np.array(list(CASES)), "weak_sizes": np.array(WEAK_SIZES, dtype=np.int32)}
    for i, b in enumerate(boxes):
        out[f"weak_boxes{i}"] = npy(b)
    for case, r in runs.items():
        names = sorted(r["losses"])
        out[f"{case}/loss_names"] = np.array(names)
        out[f"{case}/losses"] = np.array([float(r["losses"][k]) for k in names], dtype=np.float64)
        for i, (bx, lg) in enumerate(r["sup_props"]):
            out[f"{case}/sup_boxes{i}"], out[f"{case}/sup_logits{i}"] = npy(bx), npy(lg)
        want = {"lp_oicr": 3, "lp_reg": 4, "lp_pcl": 0}[case]
        assert len(r["calls"]) == want, (case, len(r["calls"]))
        for k, (lab, w) in enumerate(r["calls"]):
            out[f"{case}/oicr_labels{k}"], out[f"{case}/oicr_weights{k}"] = npy(lab), npy(w)
        print(case, {k: round(float(v), 6) for k, v in sorted(r["losses"].items())}, flush=True)
    assert all(v.dtype in (np.float32, np.float64, np.int32) or v.dtype.kind == "U" for v in out.values())
    np.savez_compressed(out_path or OUT, **out)
    print("wrote", out_path or OUT, len(out), "arrays", os.path.getsize(out_path or OUT), "bytes")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--search"]
    main(args[0] if args else None, search="--search" in sys.argv)
