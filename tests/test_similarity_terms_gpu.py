"""The similarity terms beyond 'lingual' + 'visual' on the GPU (csrc/similarity.hip): unit_similarity_static + unit_similarity_ex against
every matrix the reference's get_similarity_matrices wrote into tests/golden/similarity_terms_golden.npz, unit_similarity_bwd_ex against
its recorded autograd gradients, bit-equality with unit_similarity on the two-term plans, the model's dispatch (similarity_dict, the eval
path), a fine-tune step with a trainable box head (fused step against module-level heads) and the recorded call list of the VOC fine-tune step."""
import os
import sys

import numpy as np
import pytest
import torch

import similarity_terms_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GDIR = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GDIR)
G = np.load(os.path.join(GDIR, "similarity_terms_golden.npz"))
pytestmark = pytest.mark.gpu
NEW_ENTRIES = ("unit_similarity_static", "unit_similarity_ex", "unit_similarity_bwd_ex")
COL0, ROW0 = 5, 7          # the refinement streams sit at an offset of the logit rows / the master matrix, as in the fused Linear


def _cases():
    for name, t in ref.SUM_CASES.items():
        yield name, name, t, "Sum"
    for name, t in ref.PRODUCT_CASES.items():
        yield name, name, t, "Product"
    for h, t in ref.MIX.items():
        yield f"mix/{h}", f"mix_{h}", t, "Sum"


CASES = list(_cases())
_INPUTS = {}


def _inputs(tag, dev):
    """the fixture's tensors of one size on the device, in the layouts the kernels read (built once, never written)"""
    if tag not in _INPUTS:
        K = ref.SIZES[tag]["K"]
        logits, W = torch.from_numpy(G[f"{tag}/logits"]), torch.from_numpy(G[f"{tag}/oicr_weight"])
        r, D = logits.shape[1], W.shape[2]
        lin = torch.full((r, COL0 + 3 * (K + 1) + 3), 1e3)          # (a kernel that read outside its columns would show)
        wm = torch.full((ROW0 + 3 * (K + 1) + 2, D + 8), 1e3)
        for s in range(3):
            lin[:, COL0 + s * (K + 1):COL0 + (s + 1) * (K + 1)] = logits[s]
            wm[ROW0 + s * (K + 1):ROW0 + (s + 1) * (K + 1), :D] = W[s]
        i32 = lambda a: torch.from_numpy(np.asarray(a)).int().to(dev)
        _INPUTS[tag] = dict(K=K, lin=lin.to(dev), wm=wm.to(dev)[:, :D], base=i32(G[f"{tag}/base"]), novel=i32(G[f"{tag}/novel"]),
                            lingual=torch.from_numpy(G[f"{tag}/lingual"]).to(dev))
    return _INPUTS[tag]


def _plan(terms, combination, tag):
    from unit_amd.modeling.similarity_terms import parse_terms
    return parse_terms(terms, combination, len(G[f"{tag}/base"]))


def _forward(tag, dev, terms, combination, rows=None):
    from unit_amd import ops
    x = _inputs(tag, dev)
    plan = _plan(terms, combination, tag)
    a = ops.similarity_static(x["wm"], ROW0, 3, x["K"] + 1, x["base"], x["novel"], x["lingual"], plan)
    lin = x["lin"] if rows is None else x["lin"][:rows].contiguous()
    return ops.similarity_ex(lin, COL0, 3, x["K"] + 1, x["base"], a, ref.THRESHOLD, plan), a, plan


def _compare(got, want, want64, terms, what):
    """got [R, n, b]; want [n, b] or [R, n, b] (the reference's shapes)"""
    want = np.broadcast_to(want, got.shape)
    assert np.array_equal(got != 0, want != 0), what
    if any("WTopK" in x for x in terms):
        # WTopK's values are dot products over D, summed in another order than torch.mm's: 4 x the reference's own fp32 error against its
        # float64 evaluation, floor 1e-6
        err_ref = float(np.abs(want[0] - want64).max())
        err = float(np.abs(got - want64[None]).max())
        print(f"{what}: kernel |err| vs float64 {err:.3e}, reference fp32 {err_ref:.3e}")
        assert err <= max(4 * err_ref, 1e-6), (what, err, err_ref)
    else:
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-7, err_msg=what)


@pytest.mark.parametrize("tag", list(ref.SIZES))
@pytest.mark.parametrize("key,_id,terms,combination", CASES, ids=[c[1] for c in CASES])
def test_kernels_against_every_fixture_matrix(dev, tag, key, _id, terms, combination):
    sim, a, plan = _forward(tag, dev, terms, combination)
    got = sim.cpu().numpy()
    want, want64 = G[f"{tag}/sim/{key}"], G[f"{tag}/sim64/{key}"]
    n, b = len(G[f"{tag}/novel"]), len(G[f"{tag}/base"])
    assert got.shape == (ref.ROWS, n, b) and tuple(a.shape) == (n, b)
    if want.ndim == 3 and tag == "K80":
        got = got[:, list(ref.K80_NOVEL_ROWS)]
    _compare(got, want, want64, terms, f"{tag}/{key}")
    one = _forward(tag, dev, terms, combination, rows=1)[0].cpu().numpy()          # R = 1
    assert one.shape == (1, n, b)
    _compare(one, G[f"{tag}/sim1/{key}"] if want.ndim == 3 else want, want64, terms, f"{tag}/{key} R=1")


def _bf16_ulp(x):
    x = np.abs(x.astype(np.float64))
    return np.where(x > 0, 2.0 ** (np.floor(np.log2(np.maximum(x, 1e-300))) - 7), 0.0)


@pytest.mark.parametrize("tag", list(ref.SIZES))
@pytest.mark.parametrize("name", ref.GRAD_CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_backward_against_recorded_autograd(dev, tag, name, dtype):
    from unit_amd import ops
    x = _inputs(tag, dev)
    K = x["K"]
    sim, a, plan = _forward(tag, dev, ref.SUM_CASES[name], "Sum")
    n, b = a.shape
    dsim = torch.from_numpy(ref.upstream(ref.ROWS, n, b)).to(dev)
    dlin = ops.similarity_bwd_ex(x["lin"], COL0, 3, K + 1, x["base"], a, ref.THRESHOLD, plan, dsim, dtype)
    assert dlin.dtype == dtype and dlin.shape == x["lin"].shape
    d = dlin.float().cpu().numpy()
    want = G[f"{tag}/grad/{name}"]
    assert not d[:, :COL0].any() and not d[:, COL0 + 3 * (K + 1):].any()
    for s in range(3):
        got = d[:, COL0 + s * (K + 1):COL0 + (s + 1) * (K + 1)]
        bound = 2e-6 + 2e-4 * np.abs(want[s]) + (_bf16_ulp(want[s]) if dtype == torch.bfloat16 else 0.0)
        err = np.abs(got - want[s])
        print(f"{tag}/{name} stream {s} {dtype}: max |err| {err.max():.3e}, max |grad| {np.abs(want[s]).max():.3e}")
        assert (err <= bound).all(), (tag, name, s, float((err - bound).max()))
    assert np.abs(want).max() > 1e-4


@pytest.mark.parametrize("tag", list(ref.SIZES))
def test_backward_is_zero_without_a_per_roi_term(dev, tag):
    from unit_amd import ops
    x = _inputs(tag, dev)
    K = x["K"]
    lists = [(ref.SUM_CASES[k], "Sum") for k in ("topk3", "wtopk3", "lsda4", "l_topk3", "average", "l_average", "none", "l_none", "wtopk5_topk3")]
    lists += [(t, "Product") for t in ref.PRODUCT_CASES.values()] + [(["lingual", "VisualK-2", "Average"], "Sum"), (["visual", "None"], "Sum")]
    for terms, comb in lists:
        sim, a, plan = _forward(tag, dev, terms, comb)
        dsim = torch.from_numpy(ref.upstream(ref.ROWS, *a.shape)).to(dev)
        for dtype in (torch.float32, torch.bfloat16):
            dlin = ops.similarity_bwd_ex(x["lin"], COL0, 3, K + 1, x["base"], a, ref.THRESHOLD, plan, dsim, dtype)
            assert dlin.shape == x["lin"].shape and not dlin.any(), (terms, comb, dtype)


@pytest.mark.parametrize("tag", list(ref.SIZES))
def test_two_term_plans_give_unit_similaritys_bits(dev, tag):
    from unit_amd import ops
    x = _inputs(tag, dev)
    K = x["K"]
    for terms in (["lingual"], ["visual"], ["lingual", "visual"], []):
        plan = _plan(terms, "Sum", tag)
        assert plan.plain
        for rows in (ref.ROWS, 1):
            lin = x["lin"][:rows].contiguous()
            old = ops.similarity(lin, COL0, 3, K + 1, x["base"], x["lingual"], x["novel"].numel(), ref.THRESHOLD, *plan.key)
            a = ops.similarity_static(x["wm"], ROW0, 3, K + 1, x["base"], x["novel"], x["lingual"], plan)
            new = ops.similarity_ex(lin, COL0, 3, K + 1, x["base"], a, ref.THRESHOLD, plan)
            assert torch.equal(old, new), (tag, terms, rows, float((old - new).abs().max()))
            if plan.visual:          # ... and so does the backward, to the tolerance of its reordered reductions
                dsim = torch.from_numpy(ref.upstream(rows, *a.shape)).to(dev)
                d_old = ops.similarity_bwd(lin, COL0, 3, K + 1, x["base"], x["lingual"], x["novel"].numel(), ref.THRESHOLD, *plan.key, dsim, torch.float32)
                d_new = ops.similarity_bwd_ex(lin, COL0, 3, K + 1, x["base"], a, ref.THRESHOLD, plan, dsim, torch.float32)
                torch.testing.assert_close(d_new, d_old, rtol=2e-4, atol=2e-6)


def test_kernels_refuse_what_they_cannot_hold(dev):
    from unit_amd import ops
    from unit_amd._lib import UnitLibError
    x = _inputs("K20", dev)
    plan = _plan(["lingual", "VisualK-2"], "Sum", "K20")
    a = ops.similarity_static(x["wm"], ROW0, 3, 21, x["base"], x["novel"], x["lingual"], plan)
    with pytest.raises(UnitLibError, match="VisualK's k"):
        ops.similarity_ex(x["lin"], COL0, 3, 21, x["base"], a, ref.THRESHOLD, plan._replace(visualk=16))
    with pytest.raises(UnitLibError, match="exclude each other"):
        ops.similarity_ex(x["lin"], COL0, 3, 21, x["base"], a, ref.THRESHOLD, plan._replace(visual=True))
    with pytest.raises(UnitLibError, match="every k"):
        ops.similarity_static(x["wm"], ROW0, 3, 21, x["base"], x["novel"], x["lingual"], plan._replace(topk=16))
    with pytest.raises(ValueError, match="leave the master matrix"):
        ops.similarity_static(x["wm"], ROW0 + 3, 3, 21, x["base"], x["novel"], x["lingual"], plan)
    with pytest.raises(ValueError, match="leave the row"):
        ops.similarity_ex(x["lin"], COL0 + 4, 3, 21, x["base"], a, ref.THRESHOLD, plan)


# ---------------------------------------------------------------------------------------------------- the model
def _mask_model(seed=4):
    from unit_amd import config
    from unit_amd.modeling import build_model
    from unit_amd.synthetic import init_synthetic_weights
    cfg = config.voc_rcnn_c4_split1(50)
    cfg.MODEL.DEVICE = "cuda"
    cfg.MODEL.RPN.PRE_NMS_TOPK_TEST, cfg.MODEL.RPN.POST_NMS_TOPK_TEST = 300, 60
    cfg.MODEL.MASK_ON = True
    cfg.MODEL.ROI_HEADS.NAME, cfg.MODEL.ROI_BOX_HEAD.NAME, cfg.MODEL.ROI_HEADS.MULTI_BOX_HEAD = "WSROIHeadNoMetaWithMask", "Res5BoxHeadWithMask", False
    ft = cfg.MODEL.ROI_HEADS.FINETUNE_TERMS
    ft.CLASSIFIER, ft.BBOX, ft.MASK = list(ref.MIX["cls"]), list(ref.MIX["bbox"]), list(ref.MIX["seg"])
    cfg.MODEL.ROI_HEADS.VISUAL_ATTENTION_HEAD.VISUAL_SIMILARITY_THRESHOLD = ref.THRESHOLD
    model = build_model(cfg)
    init_synthetic_weights(model, seed=seed)
    model.eval()
    model.compute_dtype = torch.float32
    return cfg, model


def test_model_dispatch_returns_the_fixture_matrices_and_the_eval_path_runs(dev):
    """one model built from a cfg with the per-head mix; every other list is set on it (the plan is parsed from the lists as they are at
    each call). similarity_dict: with a predictor of the fixture's width holding the fixture's weights. roi_heads_inference: as built."""
    from unit_amd.modeling.inference import class_roles, similarity_dict
    from unit_amd.structures import FAST_RCNN_REGISTRY, ShapeSpec
    from unit_amd.synthetic import synthetic_batch
    tag, K = "K20", 20
    cfg, model = _mask_model()
    rh = model.roi_heads
    assert {h: p.plain for h, p in rh.term_plans().items()} == {"cls": False, "bbox": False, "seg": True}
    assert list(rh._coco_indexer) == G[f"{tag}/coco_indexer"].tolist() and list(rh._base_classes) == G[f"{tag}/base"].tolist()
    sup, _ = synthetic_batch(1, 0, hw=(96, 128), seed=7, max_gt=3)
    lists = [(k, {h: t for h in ("cls", "bbox", "seg")}, c) for k, _, t, c in CASES if not k.startswith("mix")] + [("mix", ref.MIX, "Sum")]
    with torch.no_grad():
        for key, terms, comb in lists:          # the eval path: _forward_box, transfer, detections, mask head with the 'seg' rows
            rh.terms, rh.similarity_combination = {h: list(t) for h, t in terms.items()}, comb
            out = model([{"image": sup[0]["image"], "height": 96, "width": 128}])[0]["instances"]
            assert torch.isfinite(out.scores).all() and torch.isfinite(out.pred_boxes.tensor).all(), key
    # the fixture's weak head (D = 48) in the place of the model's
    D = ref.SIZES[tag]["D"]
    full = rh.box_predictor
    bp = FAST_RCNN_REGISTRY.get(cfg.MODEL.ROI_HEADS.FAST_RCNN.NAME)(cfg, ShapeSpec(channels=D)).to(dev)
    wh = bp.weak_detector_head
    glove = torch.from_numpy(np.load(os.path.join(GDIR, "unit_golden.npz"))["glove_mean"])          # the reference's 80 x 300 embedding table
    assert glove.shape == bp.embeddings.weight.shape == full.embeddings.weight.shape
    with torch.no_grad():
        bp.embeddings.weight.copy_(glove)
        for s, l in enumerate(wh.oicr_predictors):
            l.weight.copy_(torch.from_numpy(G[f"{tag}/oicr_weight"][s]))
            l.bias.copy_(torch.from_numpy(G[f"{tag}/oicr_bias"][s]))
    bp.compute_dtype = torch.float32
    bp.prepare(torch.float32, 0)
    rh.box_predictor = bp
    rh._role_cache = None
    lin = torch.zeros((ref.ROWS, wh.group.kp), device=dev)
    for s, c in enumerate(wh.col_oicr):
        lin[:, c:c + K + 1] = torch.from_numpy(G[f"{tag}/logits"][s]).to(dev)
    # the lingual matrix: the model's own (unit_embedding_similarity, a 300-term dot product summed in another order than the reference's
    # torch.mm) agrees with the fixture's to fp32 rounding of values up to ~40; the matrices below are compared on the FIXTURE's lingual
    # matrix, as the kernel-level test compares them, so that the plain bar holds for what this pull request computes
    from unit_amd import ops
    t_ = class_roles(rh)
    ling_fix = torch.from_numpy(G[f"{tag}/lingual"]).to(dev)
    ling_own = ops.embedding_similarity(bp.embeddings.weight, t_["emb_novel"], t_["emb_base"])
    torch.testing.assert_close(ling_own, ling_fix, rtol=1e-5, atol=1e-4)
    orig = ops.embedding_similarity
    ops.embedding_similarity = lambda *a: ling_fix
    try:
        for key, terms, comb in lists:
            rh.terms, rh.similarity_combination = {h: list(t) for h, t in terms.items()}, comb
            sims = similarity_dict(rh, lin)
            for h, t in terms.items():
                fk = f"{key}/{h}" if key == "mix" else key
                _compare(sims[h].cpu().numpy(), G[f"{tag}/sim/{fk}"], G[f"{tag}/sim64/{fk}"], t, f"model {fk}")
    finally:
        ops.embedding_similarity = orig
    rh.terms = {h: ["lingual", "Visual"] for h in ("cls", "bbox", "seg")}          # edited on a built model: refused where the matrix is computed
    with pytest.raises(ValueError, match="not a similarity term"):
        similarity_dict(rh, lin)


# ---------------------------------------------------------------------------------------------------- the fine-tune step
FT_TERMS = ["lingual", "VisualK-2"]


def _ft_inputs(terms=FT_TERMS, name="mask_ft"):
    """gen_ref_step's "mask_ft" case (WSROIHeadWithMaskFineTune at reduced size: the box head trains under the fine-tune heads) or its "s2" case
    (WSROIHeadFineTune, the VOC fine-tune yaml: only the two _ft predictors train) with `terms` on every head"""
    import gen_ref_step as S
    cfg, model, sup, weak, perms, _ = S.step_inputs(name, device="cuda")
    if terms is not None:
        model.roi_heads.terms = {h: list(terms) for h in model.roi_heads.terms}
    model.train()
    for m in model.modules():
        m.compute_dtype = torch.float32
    return cfg, model, sup, perms


def test_finetune_step_fused_against_module_level_heads(dev):
    """['lingual', 'VisualK-2'] on every head, box head trainable: the fused step (rcnn.forward_train / backward_train) and the ROI heads
    called as a module in training (train_modules._HeadsFn) agree on every loss to 1e-6 and on the gradient of every trainable tensor --
    the box head's, which only its input gradient reaches, among them -- to 1e-5 of its largest entry: the bar of the existing comparison of
    the two paths (test_module_level_training_matches_the_fused_step). Against the default terms the box head's gradient moves."""
    from unit_amd.modeling.rcnn import LOSS_NAMES
    from unit_amd.structures import ImageList

    def fused(terms):
        cfg, model, sup, perms = _ft_inputs(terms)
        batch = model.pack_batch(sup, None)
        model._ensure_ready()
        cap = cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN + batch.gt_boxes.shape[1]
        roi = torch.stack([torch.cat([p, torch.arange(len(p), cap)]) for p in perms["roi"]])
        step = model.forward_train(batch, {"rpn": torch.stack(perms["rpn"]).int().to(dev), "roi": roi.int().to(dev)}, early_backward=True)
        model.backward_train(step)
        return cfg, model, step, dict(zip(LOSS_NAMES, step.losses.cpu().tolist()))
    cfg, ref_model, step, ref_losses = fused(FT_TERMS)
    ref_grads = {n: q.grad.detach().clone() for n, q in ref_model.named_parameters() if q.requires_grad}
    name = "roi_heads.box_head.res5.0.conv1.weight"
    assert name in ref_grads
    _, dflt, _, dflt_losses = fused(None)
    gd = dict(dflt.named_parameters())[name].grad
    assert (gd - ref_grads[name]).abs().max().item() > 1e-3 * gd.abs().max().item() and dflt_losses["loss_cls"] != ref_losses["loss_cls"]

    _, model, sup, perms = _ft_inputs(FT_TERMS)
    hw = tuple(sup[0]["image"].shape[-2:])
    mean, std = torch.tensor(cfg.MODEL.PIXEL_MEAN).view(1, 3, 1, 1), torch.tensor(cfg.MODEL.PIXEL_STD).view(1, 3, 1, 1)
    x = ((torch.stack([s["image"] for s in sup]) - mean) / std).to(dev)
    images, gt = ImageList(None, [hw] * len(sup)), [s["instances"] for s in sup]
    cap = cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN + max(8, (max(len(s["instances"]) for s in sup) + 7) // 8 * 8)
    features = model.backbone(x)
    model.proposal_generator.next_perm = torch.stack(perms["rpn"]).int().to(dev)
    proposals, proposal_losses = model.proposal_generator(images, features, gt)
    model.roi_heads.next_perm = torch.stack([torch.cat([p, torch.arange(len(p), cap)]) for p in perms["roi"]]).int().to(dev)
    _, losses = model.roi_heads(images, features, proposals, gt)
    losses = {**losses, **proposal_losses}
    assert set(losses) == {"loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc", "loss_mask"}
    sum(losses.values()).backward()
    for k, v in losses.items():
        assert abs(v.item() - ref_losses[k]) <= 1e-6 * max(1.0, abs(ref_losses[k])), (k, v.item(), ref_losses[k])
    checked = 0
    for n, q in model.named_parameters():
        if q.requires_grad:
            g, gr = q.grad.detach(), ref_grads[n]
            assert (g - gr).abs().max().item() <= 1e-5 * gr.abs().max().item() + 1e-8, (n, (g - gr).abs().max().item(), gr.abs().max().item())
            checked += 1
    assert checked == len(ref_grads) and any(n.startswith("roi_heads.box_head.") for n in ref_grads)


def _plan_names(rs):
    plan = next(iter(rs.plans.values()))[0]
    return [n for it in plan.items if it[0] == "calls" for n in it[3]]


def _run_steps(terms, replay, steps=3, name="s2"):
    from unit_amd import engine
    from unit_amd.solver import FlatSGD
    cfg, model, sup, _ = _ft_inputs(terms, name)
    opt = FlatSGD(model, cfg)
    out = []
    if replay:
        rs = engine.ReplayedStep(model, opt, warmup_steps=1)
        out = [rs.run(sup, None).clone() for _ in range(steps)]
        torch.cuda.synchronize()
        return out, model, rs
    for _ in range(steps):
        b = model.pack_batch(sup, None, gt_buckets=engine.GraphedStep.GT_BUCKETS)
        opt._bind()
        opt.use_device_lr(model.device)
        step = model.forward_train(b, early_backward=True)
        model.backward_train(step)
        opt.step()
        out.append(step.losses.clone())
    torch.cuda.synchronize()
    return out, model, None


def test_finetune_step_replayed_is_the_eager_step(dev):
    """three steps of the VOC fine-tune configuration with ['lingual', 'VisualK-2']: engine.ReplayedStep ends bit-equal to the eager steps, and
    its call list names the two forward entries once per step (the box head is frozen there: no similarity backward)."""
    eager, m1, _ = _run_steps(FT_TERMS, replay=False)
    got, m2, rs = _run_steps(FT_TERMS, replay=True)
    assert rs.stats == {"eager": 1, "captured": 1, "replayed": 1}
    for k, (a, b) in enumerate(zip(got, eager)):
        assert torch.isfinite(a).all() and torch.equal(a, b), (k, a.tolist(), b.tolist())
    assert torch.equal(m2.store.params, m1.store.params)
    names = _plan_names(rs)
    assert [names.count(n) for n in NEW_ENTRIES] == [1, 1, 0], [names.count(n) for n in NEW_ENTRIES]
    assert "unit_similarity" not in names and "unit_similarity_bwd" not in names


def test_replayed_step_refuses_a_finetune_step_whose_box_head_trains(dev):
    """the fused step of that configuration (the mask fine-tune yaml) makes part of its work with stock torch operators, which a call list does
    not hold: with the DEFAULT terms, on code older than the similarity terms, the replayed third step of the reduced-size case gave loss_mask
    1.073573 where the eager step has 1.492895 (MI355X). ReplayedStep says so instead of recording such a list, with any term list."""
    from unit_amd import engine
    from unit_amd.solver import FlatSGD
    for terms in (None, FT_TERMS):
        cfg, model, sup, _ = _ft_inputs(terms, "mask_ft")
        with pytest.raises(NotImplementedError, match="fine-tune step whose box head trains.*stock torch operators"):
            engine.ReplayedStep(model, FlatSGD(model, cfg), warmup_steps=1)
    cfg, model, sup, _ = _ft_inputs(FT_TERMS, "s2")          # frozen box head: taken
    engine.ReplayedStep(model, FlatSGD(model, cfg), warmup_steps=1)


def test_default_terms_record_none_of_the_new_entries(dev):
    _, _, rs = _run_steps(None, replay=True, steps=2)
    names = _plan_names(rs)
    assert len(names) > 100 and not any(n in NEW_ENTRIES for n in names), [n for n in names if n in NEW_ENTRIES]
    assert names.count("unit_similarity") == 1 and names.count("unit_similarity_bwd") == 0
