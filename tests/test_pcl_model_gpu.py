"""Weak detector TYPE "PCL" through the model: the module-level head (forward + losses + backward) against the reference's recorded losses
and logits gradients (tests/golden/pcl_targets_golden.npz), the fused training step against the same step with TYPE "OICR" (everything
the refinement streams do not touch is bit-equal) and against unit_pcl_targets + unit_pcl_loss called by hand on the step's own tensors,
the replayed step against the eager one, and one step at the baseline size."""
import ast
import os
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GDIR = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GDIR)
import pcl_targets as pt  # noqa: E402

G = np.load(os.path.join(GDIR, "pcl_targets_golden.npz"))
OLD = np.load(os.path.join(GDIR, "pcl_golden.npz"))
DENSE = [t for t in pt.tags(G) if not int(G[f"{t}/sparse"])]
DPAD = 128          # the Linear kernels are built for the model's feature widths (multiples of 128): zero columns leave every logit as it is


# ---------------------------------------------------------------------------------------------------- module level
def _head(tag, dev):
    from unit_amd import config
    from unit_amd.layers import invalidate_prepared
    from unit_amd.modeling.fast_rcnn import WeakDetectorOutputsBase
    from unit_amd.structures import ShapeSpec
    K = int(G[f"{tag}/K"])
    cfg = config.get_cfg()
    cfg.MODEL.ROI_HEADS.NUM_CLASSES = K
    wd = cfg.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR
    wd.TYPE, wd.MIL_MULTIPLIER = "PCL", 4.0             # the reference head's default multiplier, as the fixture's generator builds it
    wh = WeakDetectorOutputsBase(cfg, ShapeSpec(channels=DPAD)).to(dev)          # the fixture's D = 32 features, zero-padded (see DPAD)
    wh.compute_dtype = torch.float32
    with torch.no_grad():
        for n, p in wh.named_parameters():
            w = torch.from_numpy(G[f"{tag}/param/{n}"])
            p.zero_()
            p[..., :w.shape[-1]].copy_(w) if w.dim() > 1 else p.copy_(w)
    invalidate_prepared()
    wh.train()
    return wh, K


def _module_run(tag, dev, weights):
    from unit_amd.structures import Boxes, Instances
    wh, K = _head(tag, dev)
    sizes = G[f"{tag}/sizes"].tolist()
    props = [Instances((300, 400), proposal_boxes=Boxes(torch.from_numpy(G[f"{tag}/boxes{i}"]).to(dev))) for i in range(len(sizes))]
    targets = [torch.from_numpy(G[f"{tag}/targets{i}"]) for i in range(len(sizes))]
    x0 = torch.from_numpy(G[f"{tag}/x"])
    x = torch.cat([x0, torch.zeros(x0.shape[0], DPAD - x0.shape[1])], 1).to(dev).requires_grad_(True)
    preds, _ = wh(x)
    for t in [preds[0], preds[1]] + list(preds[2]):
        t.retain_grad()
    losses = wh.losses(preds, props, targets)
    sum(weights.get(k, 1.0) * v for k, v in losses.items()).backward()
    return preds, losses


@pytest.mark.parametrize("tag", DENSE)
def test_module_level_head_vs_reference(dev, tag):
    """loss_im_cls, loss_oicr_1..3 within rtol 1e-5 (NaN where the reference's is), refinement-logits gradients rtol 2e-4 / atol 2e-6"""
    preds, losses = _module_run(tag, dev, {})
    assert set(losses) == {"loss_im_cls", "loss_oicr_1", "loss_oicr_2", "loss_oicr_3"}
    torch.testing.assert_close(losses["loss_im_cls"].detach().cpu(), torch.from_numpy(G[f"{tag}/stable/loss_im_cls"]), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(preds[0].detach().cpu().numpy(), G[f"{tag}/classifier_logits"], rtol=1e-4, atol=1e-5)
    for it in range(3):
        print(tag, it, float(losses[f"loss_oicr_{it + 1}"].detach()), float(pt.recorded(G, OLD, tag, it, "loss")))
        torch.testing.assert_close(losses[f"loss_oicr_{it + 1}"].detach().cpu(), torch.from_numpy(pt.recorded(G, OLD, tag, it, "loss")),
                                   rtol=1e-5, atol=1e-6, equal_nan=True)
        torch.testing.assert_close(preds[2][it].grad.cpu(), torch.from_numpy(pt.recorded(G, OLD, tag, it, "grad_logits")), rtol=2e-4, atol=2e-6)


def test_module_level_refinement_gradient_ignores_the_loss_weight(dev):
    """PCLFunction.backward ignores grad_output: every loss times 3 before backward leaves the refinement gradients as they are and
    triples the MIL streams'"""
    p1, _ = _module_run("S40", dev, {})
    p3, _ = _module_run("S40", dev, {k: 3.0 for k in ("loss_im_cls", "loss_oicr_1", "loss_oicr_2", "loss_oicr_3")})
    for it in range(3):
        assert float(p1[2][it].grad.abs().max()) > 0 and torch.equal(p1[2][it].grad, p3[2][it].grad)
    for s in (0, 1):
        assert float(p1[s].grad.abs().max()) > 0
        torch.testing.assert_close(p3[s].grad, 3.0 * p1[s].grad, rtol=1e-6, atol=0)


# ---------------------------------------------------------------------------------------------------- the fused step
def _fused_step(typ, dev):
    import gen_ref_step as grs
    orig = grs.case_cfg

    def cfg_of(name, device="cpu"):
        c = orig(name, device)
        c.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR.TYPE = typ
        return c
    grs.case_cfg = cfg_of
    try:
        cfg, model, sup, weak, perms, _ = grs.step_inputs("s1", device="cuda")
    finally:
        grs.case_cfg = orig
    from unit_amd.modeling.rcnn import LOSS_NAMES
    model.train()
    model.compute_dtype = torch.float32
    batch = model.pack_batch(sup, weak)
    model._ensure_ready()
    cap = cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN + batch.gt_boxes.shape[1]
    roi = torch.stack([torch.cat([p, torch.arange(len(p), cap)]) for p in perms["roi"]])
    dperms = {"rpn": torch.stack(perms["rpn"]).int().to(dev), "roi": roi.int().to(dev)}
    wh = model.roi_heads.box_predictor.weak_detector_head
    seen, inner = {}, wh.fused_losses

    def spy(lin, rois5, valid, s, b, multihot, loss_out, grad_dtype, side_stream=None):
        seen.update(lin=lin, rois5=rois5, valid=valid, s=s, b=b, multihot=multihot)
        return inner(lin, rois5, valid, s, b, multihot, loss_out, grad_dtype, side_stream=side_stream)
    wh.fused_losses = spy
    step = model.forward_train(batch, dperms, early_backward=True)
    model.backward_train(step)
    torch.cuda.synchronize()
    del wh.fused_losses
    return model, step, seen, dict(zip(LOSS_NAMES, step.losses.clone()))


def _by_hand(wh, seen, dy_dtype=torch.float32):
    """unit_pcl_targets + unit_pcl_loss per refinement stream on the step's own lin_weak / rois / valid -> (losses [n], dy)"""
    from unit_amd import ops
    k, lin = wh.num_classes, seen["lin"]
    xr = ops.wsddn_mil(lin, wh.col_cls, wh.col_det, k, seen["valid"], seen["s"], seen["b"], seen["multihot"], wh.classifier_temp,
                       wh.detector_temp, wh.mil_multiplier)[1]
    dy = torch.zeros((lin.shape[0], wh.group.kp), dtype=dy_dtype, device=lin.device)
    out = []
    for it in range(wh.oicr_iter):
        src, col0, mode = (xr, 0, 0) if it == 0 else (lin, wh.col_oicr[it - 1], 1)
        t = ops.pcl_targets(src, col0, mode, lin, wh.col_oicr[it], 1, k, seen["rois5"], seen["valid"], seen["s"], seen["b"], seen["multihot"],
                            ldc=wh.max_pc_num * k, fg_thresh=wh.fg_threshold, bg_thresh=wh.bg_threshold,
                            graph_iou_thresh=wh.graph_iou_threshold, max_pc_num=wh.max_pc_num)
        out.append(ops.pcl_loss(lin, wh.col_oicr[it], k, seen["valid"], seen["s"], seen["b"], t["labels"][0], t["cls_weights"][0],
                                t["gt_assign"][0], t["pc_count"][0], t["pc_img_cls_weights"][0], t["pc_probs"][0], t["n_pc"][0], dy=dy,
                                dcol0=wh.col_oicr[it])[0].clone())
    return out, dy


def test_fused_step_pcl_beside_oicr_and_by_hand(dev):
    mo, so, _, lo = _fused_step("OICR", dev)
    mp, sp, seen, lp = _fused_step("PCL", dev)
    wh, k = mp.roi_heads.box_predictor.weak_detector_head, mp.roi_heads.num_classes
    for name in lo:
        if not name.startswith("loss_oicr_"):
            assert torch.equal(lo[name], lp[name]), name
    for it in range(3):
        assert torch.isfinite(lp[f"loss_oicr_{it + 1}"]) and not torch.equal(lo[f"loss_oicr_{it + 1}"], lp[f"loss_oicr_{it + 1}"])
    for c in (wh.col_cls, wh.col_det):
        assert torch.equal(so.dy_weak[:, c:c + k], sp.dy_weak[:, c:c + k])
    po, pp = dict(mo.named_parameters()), dict(mp.named_parameters())
    for n in ("roi_heads.box_predictor.cls_score_delta.weight", "roi_heads.box_predictor.bbox_pred_delta.weight"):
        assert float(pp[n].grad.abs().max()) > 0 and torch.equal(po[n].grad, pp[n].grad), n
    losses, dy = _by_hand(wh, seen, sp.dy_weak.dtype)
    for it in range(3):
        assert torch.equal(losses[it], lp[f"loss_oicr_{it + 1}"]), it
        c = wh.col_oicr[it]
        assert float(dy[:, c:c + k + 1].abs().max()) > 0 and torch.equal(dy[:, c:c + k + 1], sp.dy_weak[:, c:c + k + 1]), it


# ---------------------------------------------------------------------------------------------------- replay
def _setup(mode="bf16"):
    from unit_amd import config
    from unit_amd.modeling import build_model
    from unit_amd.synthetic import init_synthetic_weights
    cfg = config.voc_rcnn_c4_split1(50)
    cfg.MODEL.DEVICE = "cuda"
    cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = 32
    cfg.MODEL.RPN.PRE_NMS_TOPK_TRAIN, cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN = 600, 100
    cfg.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR.TYPE = "PCL"
    cfg.SOLVER.WARMUP_ITERS = 4
    cfg.SEED = 3
    model = build_model(cfg)
    init_synthetic_weights(model, seed=1)
    model.train()
    model.compute_mode = mode
    return cfg, model


def _meta_ops():
    """the operators tools/stock_ops.py counts as pure metadata / allocation (read from that file: one list)"""
    with open(os.path.join(ROOT, "tools", "stock_ops.py")) as f:
        m = re.search(r"^META = (\{.*?\})", f.read(), flags=re.S | re.M)
    return ast.literal_eval(m.group(1))


def test_replayed_pcl_step_equals_eager_and_launches_no_stock_operator(dev):
    from torch.utils._python_dispatch import TorchDispatchMode
    from unit_amd import engine
    from unit_amd.solver import FlatSGD
    from unit_amd.synthetic import synthetic_batch
    data = [synthetic_batch(2, 2, hw=(128, 192), seed=50 + i, max_gt=4) for i in range(3)]
    seq = [data[i] for i in (0, 1, 2, 1, 0, 2)]
    meta = _meta_ops()

    class Log(TorchDispatchMode):
        calls = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            parts = str(func).split(".")
            if (parts[1] if len(parts) >= 2 else parts[0]) not in meta:
                self.calls.append(str(func))
            return func(*args, **(kwargs or {}))
    cfg, m1 = _setup()
    o1 = FlatSGD(m1, cfg)
    ref = []
    for j, d in enumerate(seq):
        b = m1.pack_batch(*d, gt_buckets=engine.GraphedStep.GT_BUCKETS)
        o1._bind()
        o1.use_device_lr(m1.device)
        log = Log() if j == 3 else None          # a steady-state step: which ATen operators does the step itself still dispatch?
        if log is not None:
            log.__enter__()
        step = m1.forward_train(b, early_backward=True)
        m1.backward_train(step)
        o1.step()
        if log is not None:
            log.__exit__(None, None, None)
        ref.append(step.losses.clone())
    torch.cuda.synchronize()
    assert Log.calls == [], Log.calls
    cfg, m2 = _setup()
    o2 = FlatSGD(m2, cfg)
    rs = engine.ReplayedStep(m2, o2, warmup_steps=2)
    got = [rs.run(*d).clone() for d in seq]
    torch.cuda.synchronize()
    assert rs.stats == {"eager": 2, "captured": 1, "replayed": 3}
    plan = next(iter(rs.plans.values()))[0]
    names = [n for it in plan.items if it[0] == "calls" for n in it[3]]
    assert "unit_pcl_targets" in names and names.count("unit_pcl_loss") == 3 and "unit_oicr_targets" not in names
    for k, (a, b) in enumerate(zip(got, ref)):
        assert torch.isfinite(a).all() and torch.equal(a, b), (k, a.tolist(), b.tolist())
    assert torch.equal(m2.store.params, m1.store.params)


# ---------------------------------------------------------------------------------------------------- baseline size
def test_pcl_step_at_baseline_size(dev):
    """R101, 600 x 1000, 2 + 2 images, 512 weak RoIs per image, bf16: finite losses, loss_oicr_k equal to the by-hand composition"""
    from unit_amd import config
    from unit_amd.modeling import build_model
    from unit_amd.modeling.rcnn import LOSS_NAMES
    from unit_amd.synthetic import init_synthetic_weights, synthetic_batch
    cfg = config.voc_rcnn_c4_split1(101)
    cfg.MODEL.DEVICE = "cuda:0"
    cfg.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR.TYPE = "PCL"
    cfg.SEED = 0
    model = build_model(cfg)
    init_synthetic_weights(model, seed=1)
    model.train()
    model.compute_mode = "bf16"
    sup, weak = synthetic_batch(2, 2, seed=100)
    batch = model.pack_batch(sup, weak)
    wh = model.roi_heads.box_predictor.weak_detector_head
    seen, inner = {}, wh.fused_losses

    def spy(lin, rois5, valid, s, b, multihot, loss_out, grad_dtype, side_stream=None):
        seen.update(lin=lin, rois5=rois5, valid=valid, s=s, b=b, multihot=multihot)
        return inner(lin, rois5, valid, s, b, multihot, loss_out, grad_dtype, side_stream=side_stream)
    wh.fused_losses = spy
    step = model.forward_train(batch, early_backward=True)
    model.backward_train(step)
    torch.cuda.synchronize()
    del wh.fused_losses
    losses = dict(zip(LOSS_NAMES, step.losses.clone()))
    assert seen["s"] == 512 and seen["b"] == 2
    assert torch.isfinite(step.losses).all(), losses
    hand, _ = _by_hand(wh, seen)
    for it in range(3):
        assert float(losses[f"loss_oicr_{it + 1}"]) > 0 and torch.equal(hand[it], losses[f"loss_oicr_{it + 1}"]), it
