"""MODEL.ROI_BOX_HEAD.POOLER_TYPE "ROIPool" and "ROIAlign" through the model: the S1 step, inference, the weak-only trainer, the replayed
and the graphed step -- against the CPU oracle with its `roi_align` replaced by the pooler under test (roi_pool_ref.roi_pool, or the
oracle's own RoIAlign with aligned=False), on the small configuration of test_step_gpu.py (R50, 32 RoIs per image, 128 x 192, fp32).

A max pooler is discontinuous in the box: a last-bit difference between two decodings of an RPN output can move a window by a pixel without
either side being wrong. The step and inference tests therefore run on GIVEN proposals on the 4-px lattice (roi_pool_cases.py), handed to
both sides; the weak-only test hands the oracle the boxes the device's own RPN produced. Tolerances are test_s1_step_parity_fp32's: losses
1e-4, gradients 2e-3 of their maximum. On the ROIPool step the device's selection is also compared with the reference pooler run on the
device's own res4 map: on identical input the two must not disagree anywhere."""
import pytest
import torch

import roi_pool_cases as pc
import roi_pool_ref as ref
import unit_oracle as orc
from unit_amd import config, engine
from unit_amd.modeling import build_model
from unit_amd.modeling.rcnn import LOSS_NAMES as _ALL_LOSS_NAMES
from unit_amd.solver import FlatSGD
from unit_amd.synthetic import init_synthetic_weights, synthetic_batch

pytestmark = pytest.mark.gpu

LOSS_NAMES = _ALL_LOSS_NAMES[:8]
HW = (128, 192)
POST = 100


def small_cfg(pooler, warmup=None):
    c = config.voc_rcnn_c4_split1(50)
    c.MODEL.DEVICE = "cuda"
    c.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = 32
    c.MODEL.RPN.PRE_NMS_TOPK_TRAIN, c.MODEL.RPN.POST_NMS_TOPK_TRAIN = 600, POST
    c.MODEL.ROI_BOX_HEAD.POOLER_TYPE = pooler
    c.SEED = 3
    if warmup is not None:
        c.SOLVER.WARMUP_ITERS = warmup
    return c


def _model(pooler, mode="fp32", seed=1, warmup=None):
    cfg = small_cfg(pooler, warmup)
    model = build_model(cfg)
    init_synthetic_weights(model, seed=seed)
    model.train()
    model.compute_mode = mode
    return cfg, model


def _patch_pooler(monkeypatch, pooler):
    if pooler == "ROIPool":
        monkeypatch.setattr(orc, "roi_align", ref.roi_pool)
    elif pooler == "ROIAlign":
        plain = orc.roi_align
        monkeypatch.setattr(orc, "roi_align", lambda feat, rois, out_size=14, spatial_scale=1.0 / 16, sampling_ratio=0, aligned=True:
                            plain(feat, rois, out_size, spatial_scale, sampling_ratio, False))


def _patch_proposals(monkeypatch, groups):
    """unit_oracle.find_top_rpn_proposals -> the given lists of (boxes, logits), one list per call in call order"""
    calls = iter(groups)
    monkeypatch.setattr(orc, "find_top_rpn_proposals", lambda *a, **k: next(calls))


def _pack(plist, dev):
    props, sc, cnt = torch.zeros(len(plist), POST, 4), torch.zeros(len(plist), POST), torch.zeros(len(plist), dtype=torch.int32)
    for i, (bx, lg) in enumerate(plist):
        props[i, : len(bx)], sc[i, : len(bx)], cnt[i] = bx, lg, len(bx)
    return props.to(dev), sc.to(dev), cnt.to(dev)


def _oracle_params(model):
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    return {k: v.detach().cpu().clone().contiguous().requires_grad_(k in trainable) for k, v in model.state_dict().items()}


def _ocfg(cfg, **kw):
    d = dict(depth=cfg.MODEL.RESNETS.DEPTH, num_classes=cfg.MODEL.ROI_HEADS.NUM_CLASSES, novel_classes=list(cfg.DATASETS.FEWSHOT.NOVEL_CLASSES_ID),
             base_classes=list(cfg.DATASETS.FEWSHOT.BASE_CLASSES_ID), coco_indexer=orc.VOC_COCO_INDEXER, pixel_mean=cfg.MODEL.PIXEL_MEAN,
             pixel_std=cfg.MODEL.PIXEL_STD, rois_per_image=cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE,
             pre_nms_topk=cfg.MODEL.RPN.PRE_NMS_TOPK_TRAIN, post_nms_topk=cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN, multi_box_head=True)
    d.update(kw)
    return d


_ORACLE_STEPS = {}


def _oracle_step(monkeypatch, pooler, model, cfg, sup, weak, perms, props):
    """the oracle's S1 step under `pooler` on the given proposals -> (losses, gradients, aux); one run per pooler type, shared by the tests
    (same weights, data and permutations in all of them), never written"""
    if pooler not in _ORACLE_STEPS:
        _patch_pooler(monkeypatch, pooler)
        _patch_proposals(monkeypatch, [props[:2], props[2:]])
        p = _oracle_params(model)
        operms = dict(rpn=[x.long().cpu() for x in perms["rpn"]], roi=[x.long().cpu() for x in perms["roi"]])
        losses, aux = orc.step_losses(p, [x["image"] for x in sup], [x["instances"].gt_boxes.tensor for x in sup],
                                      [x["instances"].gt_classes for x in sup], [x["image"] for x in weak],
                                      [x["instances"].gt_classes for x in weak], operms, _ocfg(cfg))
        sum(losses.values()).backward()
        _ORACLE_STEPS[pooler] = ({k: v.item() for k, v in losses.items()}, {k: v.grad for k, v in p.items() if v.grad is not None},
                                 dict(anchor_labels=aux["anchor_labels"], sampled=aux["sampled"], weak_boxes=aux["weak_boxes"]))
    return _ORACLE_STEPS[pooler]


def _device_step(pooler, pool_mode, mode="fp32"):
    cfg, model = _model(pooler, mode)
    model.roi_heads.pool_mode = pool_mode
    sup, weak = synthetic_batch(2, 2, hw=HW, seed=5, max_gt=4)
    batch = model.pack_batch(sup, weak)
    model._ensure_ready()
    perms = model.sampling_permutations(2, 8 * 12 * 15, POST + batch.gt_boxes.shape[1])
    props = pc.lattice_proposals(4, POST, HW, seed=23)
    step = model.forward_train(batch, perms, proposals=_pack(props, model.device))
    model.backward_train(step)
    return cfg, model, sup, weak, perms, props, step


def _check_against_oracle(model, step, ref_losses, ref_grads, aux, grad_bar):
    got = dict(zip(LOSS_NAMES, step.losses.cpu().tolist()))
    assert torch.equal(step.anchor_labels.cpu(), torch.stack(aux["anchor_labels"]))
    for i in range(2):          # the proposals were given: the sampled boxes are the same bits on both sides
        rb = aux["sampled"][i]["boxes"]
        sl = slice(i * 32, i * 32 + len(rb))
        assert torch.equal(step.rois[sl, 1:].cpu(), rb), i
        assert torch.equal(step.roi_cls[sl].cpu().long(), aux["sampled"][i]["gt_classes"])
        wb = aux["weak_boxes"][i]
        assert torch.equal(step.rois[64 + i * 32: 64 + i * 32 + len(wb), 1:].cpu(), wb), i
    print({k: (got[k], ref_losses[k]) for k in LOSS_NAMES})
    worst, checked = 0.0, 0
    errs = {}
    for name, prm in model.named_parameters():
        if not prm.requires_grad:
            continue
        g_ref = ref_grads[name]
        scale = g_ref.abs().max().item() + 1e-12
        errs[name] = ((prm.grad.detach().cpu() - g_ref).abs().max().item(), scale)
        worst = max(worst, max(errs[name][0] - 1e-7, 0.0) / scale)          # (the bar's absolute term: tensors whose gradient is zero by construction)
        checked += 1
    print("worst gradient error / max", worst)
    for k in LOSS_NAMES:
        assert abs(got[k] - ref_losses[k]) <= 1e-4 * max(1.0, abs(ref_losses[k])), (k, got[k], ref_losses[k])
    for name, (err, scale) in errs.items():
        assert err <= grad_bar * scale + 1e-7, (name, err, scale)
    assert checked == 72          # R50: res3 13 + res4 19 + 2 x res5 10 + rpn 6 + heads 14 trainable tensors


def _selection_disagreement(model, step):
    """the reference pooler on the device's own fp32 res4 map against what the device selected: -> number of differing argmax entries"""
    rh = model.roi_heads
    osz, stp = rh.pool_out
    o, a = ref.forward(step.feat.cpu().numpy(), step.rois.cpu().numpy(), rh.pooler_resolution, bins=pc.bins(rh.pooler_resolution, osz, stp))
    return int((torch.from_numpy(a) != step.pool_argmax.cpu()).sum()), a.size


# ---------------------------------------------------------------------------------------------------- (a) S1 step parity
@pytest.mark.parametrize("pool_mode", ["strided", "full"])
@pytest.mark.parametrize("pooler", ["ROIPool", "ROIAlign"])
def test_s1_step_parity_fp32(dev, monkeypatch, pooler, pool_mode):
    cfg, model, sup, weak, perms, props, step = _device_step(pooler, pool_mode)
    if pooler == "ROIPool":
        assert step.pool_argmax is not None and step.pool_argmax.dtype == torch.int32 and step.pool_argmax.shape[:3] == (128,) + 2 * (model.roi_heads.pool_out[0],)
        bad, n = _selection_disagreement(model, step)
        print("argmax entries that differ from the reference pooler on the device's map:", bad, "of", n)
        assert bad == 0
    else:
        assert step.pool_argmax is None
    ref_losses, ref_grads, aux = _oracle_step(monkeypatch, pooler, model, cfg, sup, weak, perms, props)
    _check_against_oracle(model, step, ref_losses, ref_grads, aux, 2e-3)


# ---------------------------------------------------------------------------------------------------- (b) inference
def test_inference_parity_roi_pool_fp32(dev, monkeypatch):
    from unit_amd.structures import Boxes, Instances
    cfg = small_cfg("ROIPool")
    model = build_model(cfg)
    init_synthetic_weights(model, seed=4)
    with torch.no_grad():   # make the class scores spread out so that several classes pass the 0.05 threshold
        g = torch.Generator().manual_seed(11)
        model.roi_heads.box_predictor.cls_score_delta.weight.copy_(torch.randn(21, 2048, generator=g) * 0.02)
    model.eval()
    model.compute_dtype = torch.float32
    sup, _ = synthetic_batch(1, 0, hw=HW, seed=8)
    (boxes, logits), = pc.lattice_proposals(1, 80, HW, seed=29)
    inp = [{"image": sup[0]["image"], "height": 256, "width": 384, "proposals": Instances(HW, proposal_boxes=Boxes(boxes), objectness_logits=logits)}]
    out = model(inp)[0]["instances"]
    p = {k: v.detach().cpu().clone().contiguous() for k, v in model.state_dict().items()}
    _patch_pooler(monkeypatch, "ROIPool")
    _patch_proposals(monkeypatch, [[(boxes, logits)]])
    b, s, c, r, aux = orc.inference(p, sup[0]["image"], _ocfg(cfg), out_hw=(256, 384))
    assert len(b) > 3
    assert len(out) == len(b), (len(out), len(b))
    assert torch.equal(out.pred_classes.cpu(), c)
    assert torch.equal(out._roi_index.cpu().long(), r)
    assert torch.allclose(out.scores.cpu(), s, rtol=1e-4, atol=1e-5)
    assert torch.allclose(out.pred_boxes.tensor.cpu(), b, rtol=1e-4, atol=2e-2)


# ---------------------------------------------------------------------------------------------------- (c) weak-only
def test_trainer_only_weak_roi_pool(dev, monkeypatch):
    """three TrainerOnlyWeak iterations under ROIPool; the first iteration's losses against the oracle's weak half (unit_oracle.step_losses'
    lines for the weak batch) under the patched pooler, on the boxes the device's RPN produced"""
    _, weak = synthetic_batch(1, 2, hw=HW, seed=5, max_gt=4)
    cfg, m1 = _model("ROIPool")
    c = m1.forward_train_only_weak(m1.pack_batch(None, weak))
    m1.backward_train_only_weak(c)
    assert c.pool_argmax is not None and tuple(c.pool_argmax.shape) == (c.rw, 7, 7, 1024)
    rh = m1.roi_heads
    sw = rh.batch_size_per_image // rh.weak_divisor
    rois, valid = c.rois.cpu(), c.weak_valid.cpu() == 0          # (unit_first_k_rois: 0 = a proposal, -1 = an unused slot)
    wboxes = [rois[i * sw:(i + 1) * sw][valid[i * sw:(i + 1) * sw], 1:].contiguous() for i in range(2)]
    assert all(len(b) > 4 for b in wboxes)
    _patch_pooler(monkeypatch, "ROIPool")
    p = _oracle_params(m1)
    with torch.no_grad():
        wx, _ = orc.preprocess_image([x["image"] for x in weak], cfg.MODEL.PIXEL_MEAN, cfg.MODEL.PIXEL_STD)
    wfeat = orc.resnet_c4(wx, p, 50, "backbone.")
    wbf = orc.res5_head(orc.roi_align(wfeat, orc.boxes_to_rois(wboxes)), p, "roi_heads.weak_box_head")
    cs, ds, oicr = orc.weak_head_forward_train(wbf, p, "roi_heads.box_predictor.weak_detector_head")
    want = orc.weak_losses(cs, ds, oicr, wboxes, [x["instances"].gt_classes for x in weak], num_classes=cfg.MODEL.ROI_HEADS.NUM_CLASSES)
    got = dict(zip(m1.loss_names, c.losses.cpu().tolist()))
    print({k: (got[k], v.item()) for k, v in want.items()})
    assert sorted(want) == ["loss_im_cls", "loss_oicr_1", "loss_oicr_2", "loss_oicr_3"]
    for k, v in want.items():
        assert abs(got[k] - v.item()) <= 1e-4 * max(1.0, abs(v.item())), (k, got[k], v.item())
    _, a_ref = ref.forward(c.feat.cpu().numpy(), rois.numpy(), 14, bins=pc.bins(14, 7, 2))          # the reference pooler on the device's own map
    assert torch.equal(torch.from_numpy(a_ref), c.pool_argmax.cpu())
    # the trainer: same weights, same data -> the same first step; then two more
    cfg, m2 = _model("ROIPool")
    tr = engine.TrainerOnlyWeak(cfg, m2)
    start = m2.store.params.clone() if m2.store is not None else None
    seen = []
    for _ in range(3):
        tr.run_step(None, weak)
        seen.append(tr.last_losses.cpu().clone())
    assert torch.equal(seen[0], c.losses.cpu())
    assert all(torch.isfinite(l).all() for l in seen) and not torch.equal(seen[0], seen[2])
    assert start is None or not torch.equal(start, m2.store.params)


# ---------------------------------------------------------------------------------------------------- (d) replay and graph
def _eager_run(seq):
    cfg, m = _model("ROIPool", "bf16", warmup=4)
    o = FlatSGD(m, cfg)
    losses = []
    for d in seq:
        b = m.pack_batch(*d, gt_buckets=engine.GraphedStep.GT_BUCKETS)
        o._bind()
        o.use_device_lr(m.device)
        step = m.forward_train(b, early_backward=True)
        m.backward_train(step)
        o.step()
        losses.append(step.losses.clone())
    torch.cuda.synchronize()
    return m, losses


@pytest.mark.parametrize("kind", ["replay", "graph"])
def test_replayed_and_graphed_step_equal_eager_roi_pool(dev, kind):
    """one eager step, the recording / capture, then two re-issued steps on other data than at the recording, the allocator churned in
    between (the argmax buffer belongs to the step's memory pool like `pooled`): losses of every step and the weights after four, bit for bit"""
    data = [synthetic_batch(2, 2, hw=HW, seed=50 + i, max_gt=4) for i in range(2)]
    seq = [data[i] for i in (0, 1, 0, 1)]
    m1, want = _eager_run(seq)
    cfg, m2 = _model("ROIPool", "bf16", warmup=4)
    o2 = FlatSGD(m2, cfg)
    runner = (engine.ReplayedStep if kind == "replay" else engine.GraphedStep)(m2, o2, warmup_steps=1)
    got = []
    for d in seq:
        got.append(runner.run(*d).clone())
        junk = [torch.full((1 << 18,), float("nan"), device=dev) for _ in range(8)]
        del junk
    torch.cuda.synchronize()
    assert runner.stats == {"eager": 1, "captured": 1, "replayed": 2}
    if kind == "replay":
        names = [n for it in next(iter(runner.plans.values()))[0].items if it[0] == "calls" for n in it[3]]
        assert names.count("unit_roi_pool_fwd") == 1 and names.count("unit_roi_pool_bwd_gather") == 2 and "unit_roi_align_fwd" not in names
    for k, (a, b) in enumerate(zip(got, want)):
        assert torch.isfinite(a).all() and torch.equal(a, b), (k, a.tolist(), b.tolist())
    assert torch.equal(m2.store.params, m1.store.params)


# ---------------------------------------------------------------------------------------------------- (e) ROIAlignV2 unchanged
def _v2_step():
    cfg, model, *_, step = _device_step("ROIAlignV2", "strided")
    assert step.pool_argmax is None
    return step.losses.cpu().clone(), model.store.grads.cpu().clone()


def test_roi_align_v2_step_does_not_see_a_roi_pool_model(dev):
    """one ROIAlignV2 step before and one after a ROIPool model was built and stepped in the same process: losses and the whole flat
    gradient bit for bit (no buffer of one pooler leaks into the other)"""
    l0, g0 = _v2_step()
    _, mp, *_, sp = _device_step("ROIPool", "strided")
    assert torch.isfinite(sp.losses).all() and sp.pool_argmax is not None
    l1, g1 = _v2_step()
    assert torch.equal(l0.view(torch.int32), l1.view(torch.int32)) and torch.equal(g0.view(torch.int32), g1.view(torch.int32))
    assert not torch.equal(l0, sp.losses.cpu())          # (and the two poolers are not the same function)


# ---------------------------------------------------------------------------------------------------- (f) bf16x3
def test_roi_pool_under_bf16x3_is_a_max_over_the_merged_map(dev, monkeypatch):
    """compute_mode "bf16x3" is NOT refused: the pooler never sees the hi / lo planes -- the step hands it the merged fp32 copy of the res4
    map (ops.as_f32, as it does for RoIAlign), so the max is over whole values. Same bars as test_step_gpu.test_s1_step_parity_bf16x3:
    losses 1e-4, gradients 1e-2 of the tensor's largest entry."""
    cfg, model, sup, weak, perms, props, step = _device_step("ROIPool", "strided", mode="bf16x3")
    assert step.feat.dtype == torch.float32 and type(step.feat) is torch.Tensor
    bad, n = _selection_disagreement(model, step)
    assert bad == 0, (bad, n)
    ref_losses, ref_grads, aux = _oracle_step(monkeypatch, "ROIPool", model, cfg, sup, weak, perms, props)
    _check_against_oracle(model, step, ref_losses, ref_grads, aux, 1e-2)


# ---------------------------------------------------------------------------------------------------- module-level heads
def test_module_level_weak_heads_equal_the_fused_step_roi_pool(dev):
    """WSROIHeadNoMeta.forward(..., train_only_weak=True) in training mode under ROIPool (train_modules._WeakHeadsFn carries the argmax from
    its forward to its backward) on the fused weak-only step's own feature map and proposals: losses within 1e-6, head gradients within
    1e-5 of their largest entry (the bars of test_only_weak_gpu.test_module_level_roi_heads_equal_the_fused_step), a gradient into the map"""
    from unit_amd import ops
    from unit_amd.structures import Boxes, ImageList, Instances
    _, weak = synthetic_batch(1, 2, hw=HW, seed=5, max_gt=4)
    cfg, model = _model("ROIPool")
    rh = model.roi_heads
    rh.compute_dtype = torch.float32
    step = model.forward_train_only_weak(model.pack_batch(None, weak))
    model.backward_train_only_weak(step)
    torch.cuda.synchronize()
    fused = dict(zip(model.loss_names, step.losses.cpu().tolist()))
    head_params = {n: q for n, q in rh.named_parameters() if q.requires_grad}
    g_fused = {n: q.grad.detach().clone() for n, q in head_params.items()}
    props, _, pcount = step.proposals
    sizes = step.image_sizes
    feats = ops.nhwc_to_nchw(ops.as_f32(step.feat).contiguous()).requires_grad_(True)
    weak_props = [Instances(tuple(sizes[i]), proposal_boxes=Boxes(props[i, :int(pcount[i])].clone())) for i in range(len(weak))]
    images = ImageList(feats, [tuple(s) for s in sizes])
    for q in head_params.values():
        q.grad.zero_()          # the module-level nodes ACCUMULATE into .grad (torch semantics)
    res, losses = rh(None, None, None, None, weak_images=images, weak_features={"res4": feats}, weak_proposals=weak_props,
                     weak_targets=[x["instances"].gt_classes.to(dev) for x in weak], train_only_weak=True)
    assert res is None and sorted(losses) == ["loss_im_cls", "loss_oicr_1", "loss_oicr_2", "loss_oicr_3"]
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    for k, v in losses.items():
        assert abs(v.item() - fused[k]) <= 1e-6 * max(1.0, abs(fused[k])), (k, v.item(), fused[k])
    checked = 0
    for n, q in head_params.items():
        ref_g = g_fused[n]
        if not ref_g.any():          # the tensors no weak loss reaches
            assert not q.grad.any(), n
            continue
        assert (q.grad - ref_g).abs().max().item() <= 1e-5 * ref_g.abs().max().item() + 1e-8, n
        checked += 1
    assert checked >= 18 and feats.grad is not None and torch.isfinite(feats.grad).all() and feats.grad.abs().sum().item() > 0
