"""The two switchable box-regression losses on the device: unit_box_reg_loss_ex / unit_rpn_loss_ex (smooth-L1 with a beta, GIoU) against
tests/golden/box_loss_golden.npz (the reference's own FastRCNNOutputsReduction.box_reg_loss and WSRPN.losses), their agreement with the plain
exports at (smooth_l1, 0), and MODEL.RPN.* / MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE, SMOOTH_L1_BETA through the model: fused step, module-level
training, replayed step, baseline size.

The tolerance of the kernel tests is not a chosen number: the kernel's loss and gradient are compared with the fixture's float64 evaluation, and
may deviate from it by 4 x what the fp32 reference itself deviates from it in that case (`dev_*`; the 4 covers an expf / division that rounds
another way than torch's), or by one fp32 ulp of the largest value compared where the reference happens to be closer than that.
MEASURED (worst error / bar over the cases of each kind, MI355X): see test_box_kernel_vs_reference / test_rpn_kernel_vs_reference."""
import ast
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GDIR = os.path.join(ROOT, "tests", "golden")
G = np.load(os.path.join(GDIR, "box_loss_golden.npz"))
BOX_SHAPES = ("K20_R1", "K20_R65", "K80_R257", "K20_R700", "K20_R65_nofg")
BOX_KINDS = ("giou", "sl1_b1e-6", "sl1_b0.111", "sl1_b1")
RPN_KINDS = ("giou", "giou_w", "sl1_b1e-6", "sl1_b0.111_w", "sl1_b1")
BOX_WEIGHTS = (10.0, 10.0, 5.0, 5.0)
JUNK = 9.0          # what the columns hold that the kernels must neither read nor write


def T(k):
    return torch.from_numpy(G[k])


def _type_of(kind):
    return "giou" if kind.startswith("giou") else "smooth_l1"


def _ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def _bar(dev, largest):
    return max(4.0 * float(dev), _ulp32(largest))


# ---------------------------------------------------------------------------------------------------- box head kernel
def _box_inputs(shape, kind, dev):
    K = int(G[f"box/{shape}/K"])
    labels, rois5, gt, d4 = T(f"box/{shape}/labels"), T(f"box/{shape}/rois5"), T(f"box/{shape}/gt"), T(f"box/{shape}/{kind}/deltas")
    R, col0 = labels.shape[0], 3
    bbox = torch.full((R, 4 * K + 8), JUNK)          # ld wider than 4K, col0 != 0; only the gt class's four columns are the fixture's
    fg = ((labels >= 0) & (labels < K)).nonzero()[:, 0]
    cols = col0 + 4 * labels[fg].long()[:, None] + torch.arange(4)
    bbox[fg[:, None], cols] = d4[fg]
    return K, R, col0, fg, cols - col0, bbox.to(dev), labels.to(dev), rois5.to(dev), gt.to(dev)


def _box_run(shape, kind, dev, dy_dtype=torch.float32, want_dy=True, raw=None):
    """-> (loss [1], dy [R, 4K + 9] or None); raw = (loss_type, beta): straight through unit_box_reg_loss_ex"""
    from unit_amd import ops
    K, R, col0, _, _, bbox, labels, rois5, gt = _box_inputs(shape, kind, dev)
    dy = torch.full((R, 4 * K + 9), JUNK, dtype=dy_dtype, device=dev) if want_dy else None
    if raw is None:
        loss = ops.box_reg_loss(bbox, col0, K, labels, rois5, gt, BOX_WEIGHTS, dy=dy, dcol0=2, loss_type=_type_of(kind), beta=float(G[f"box/{shape}/{kind}/beta"]))
    else:
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        w = (ctypes.c_float * 4)(*BOX_WEIGHTS)
        ops.check(ops.lib().unit_box_reg_loss_ex(ops._p(bbox), bbox.shape[1], col0, K, ops._p(labels), ops._p(rois5), ops._p(gt), w, R, 1.0, ops._p(loss),
                                                 ops._p(dy), ops.dt(dy.dtype) if dy is not None else 0, dy.shape[1] if dy is not None else 0, 2,
                                                 ops._p(ops._loss_acc(bbox.device)), raw[0], raw[1], ops._s()), "box_reg_loss_ex")
    torch.cuda.synchronize()
    return loss.cpu(), (dy.cpu() if dy is not None else None)


@pytest.mark.parametrize("kind", BOX_KINDS)
@pytest.mark.parametrize("shape", BOX_SHAPES)
def test_box_kernel_vs_reference(dev, shape, kind):
    """loss and fp32 gradient within the bar of the module docstring; label -1 / background rows and every column but the gt class's four
    are exactly zero, the columns beside the 4K block untouched; dy = None gives the same loss; two runs are bit-equal.
    MEASURED worst error / bar: (over the five shapes) giou loss 0.25 grad 0.76; sl1_b1e-6 loss 0.07 grad 0.25; sl1_b0.111 loss 0.14 grad 0.00; sl1_b1 loss 0.23 grad 0.01"""
    pre = f"box/{shape}/{kind}"
    K, R, _, fg, cols, *_ = _box_inputs(shape, kind, "cpu")
    loss, dy = _box_run(shape, kind, dev)
    l64, g64 = float(G[f"{pre}/loss/f64"]), G[f"{pre}/grad/f64"]
    bar_l = _bar(G[f"{pre}/dev_loss"], l64)
    bar_g = _bar(G[f"{pre}/dev_grad"], np.abs(g64).max() if g64.size else 0.0)
    block = dy[:, 2:2 + 4 * K].double()
    got = torch.zeros(R, 4, dtype=torch.float64)
    got[fg] = block[fg[:, None], cols]
    err_l, err_g = abs(float(loss) - l64), float((got - torch.from_numpy(g64)).abs().max())
    print(f"{pre}: loss {float(loss):.9g} err {err_l:.3g} bar {bar_l:.3g} ratio {err_l / bar_l if bar_l else 0:.2f} | "
          f"grad err {err_g:.3g} bar {bar_g:.3g} ratio {err_g / bar_g if bar_g else 0:.2f}")
    assert err_l <= bar_l and err_g <= bar_g
    rest = block.clone()
    rest[fg[:, None], cols] = 0
    assert float(rest.abs().max()) == 0.0          # -1 rows, background rows, the other classes' columns
    assert bool((dy[:, :2] == JUNK).all()) and bool((dy[:, 2 + 4 * K:] == JUNK).all())
    if len(fg):
        assert float(block[fg].abs().max()) > 0
    assert torch.equal(_box_run(shape, kind, dev, want_dy=False)[0], loss)
    loss2, dy2 = _box_run(shape, kind, dev)
    assert torch.equal(loss2, loss) and torch.equal(dy2, dy)


@pytest.mark.parametrize("kind", BOX_KINDS)
@pytest.mark.parametrize("shape", ("K20_R65", "K20_R700"))
def test_box_kernel_bf16_gradient(dev, shape, kind):
    """the bf16 gradient is the fp32 gradient rounded to bf16, to within one bf16 ulp; the loss does not depend on the gradient's dtype"""
    K = int(G[f"box/{shape}/K"])
    l32, d32 = _box_run(shape, kind, dev)
    l16, d16 = _box_run(shape, kind, dev, dy_dtype=torch.bfloat16)
    assert torch.equal(l16, l32)
    _one_bf16_ulp(d16[:, 2:2 + 4 * K], d32[:, 2:2 + 4 * K])


def _one_bf16_ulp(got, want32):
    want = want32.to(torch.bfloat16).float()
    ulp = torch.where(want == 0, torch.zeros_like(want), torch.exp2(torch.floor(torch.log2(want.abs().clamp(min=1e-38))) - 7))
    assert bool(((got.float() - want).abs() <= ulp).all())
    assert float(want.abs().max()) > 0


@pytest.mark.parametrize("shape", BOX_SHAPES)
def test_box_ex_at_smooth_l1_beta_0_is_the_plain_export(dev, shape):
    """(UNIT_BOXLOSS_SMOOTH_L1, 0.0f) through unit_box_reg_loss_ex: bit for bit unit_box_reg_loss; a beta below 1e-5 is L1 too (the same
    gradient, bit for bit), summed by the general smooth-L1 body"""
    from unit_amd import ops
    K, R, col0, _, _, bbox, labels, rois5, gt = _box_inputs(shape, "sl1_b1e-6", dev)
    for dtype in (torch.float32, torch.bfloat16):
        dy = torch.full((R, 4 * K + 9), JUNK, dtype=dtype, device=dev)
        plain = ops.box_reg_loss(bbox, col0, K, labels, rois5, gt, BOX_WEIGHTS, dy=dy, dcol0=2).cpu()
        loss, dy_ex = _box_run(shape, "sl1_b1e-6", dev, dy_dtype=dtype, raw=(0, 0.0))
        assert torch.equal(loss, plain) and torch.equal(dy_ex, dy.cpu()), dtype
        loss, dy_ex = _box_run(shape, "sl1_b1e-6", dev, dy_dtype=dtype, raw=(0, 1e-6))
        assert torch.equal(dy_ex, dy.cpu()), dtype          # (its loss: test_box_kernel_vs_reference, against float64)


# ---------------------------------------------------------------------------------------------------- RPN kernel
def _rpn_inputs(kind, dev):
    A = int(G["rpn/A"])
    logits, deltas = T(f"rpn/{kind}/logits"), T(f"rpn/{kind}/deltas")
    B, N = logits.shape
    head = torch.full((B, N // A, 80), JUNK)          # ld 80 for 5A = 75 columns, the deltas one column further right than the model has them
    head[:, :, :A] = logits.reshape(B, N // A, A)
    head[:, :, A + 1:5 * A + 1] = deltas.reshape(B, N // A, 4 * A)
    return A, B, N, head.to(dev), T("rpn/labels").to(dev), T("rpn/match").to(dev), T("rpn/gt").to(dev), T("rpn/anchors").to(dev)


def _rpn_run(kind, dev, grad_dtype=torch.float32, raw=None):
    from unit_amd import ops
    A, B, N, head, labels, match, gt, anchors = _rpn_inputs(kind, dev)
    norm = int(G["rpn/batch_size_per_image"]) * B
    weights = tuple(float(v) for v in G[f"rpn/{kind}/weights"])
    if raw is None:
        loss2, dhead = ops.rpn_loss(head, A, A + 1, labels, match, gt, anchors, norm, grad_dtype, weights=weights, loss_type=_type_of(kind),
                                    beta=float(G[f"rpn/{kind}/beta"]))
    else:
        loss2 = torch.empty(2, dtype=torch.float32, device=dev)
        dhead = torch.empty(head.shape, dtype=grad_dtype, device=dev)
        nbytes = ops.lib().unit_rpn_loss_scratch_bytes(B, N)
        scratch = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
        ops.check(ops.lib().unit_rpn_loss_ex(ops._p(head), 80, A, A + 1, ops._p(labels), ops._p(match), ops._p(gt), gt.shape[1], ops._p(anchors), B, N,
                                             float(norm), 1.0, weights[0], weights[1], ops._p(loss2), ops._p(dhead), ops.dt(grad_dtype), ops._p(scratch),
                                             nbytes, raw[0], raw[1], ops._s()), "rpn_loss_ex")
    torch.cuda.synchronize()
    return loss2.cpu(), dhead.cpu()


@pytest.mark.parametrize("kind", RPN_KINDS)
def test_rpn_kernel_vs_reference(dev, kind):
    """both losses and the fp32 gradients of logits and deltas within the bar of the module docstring (525 anchors: three workgroups per image,
    the last partial; one image without a positive; loss weights (0.5, 2) in the _w cases); anchors with label -1 get zero gradient in every
    column, label 0 in the four delta columns; pad columns are zero; two runs are bit-equal.
    MEASURED worst error / bar: giou loc 0.25 cls 0.04 d/deltas 0.25 d/logits 0.25; giou_w loc 0.25 cls 0.06 d/deltas 0.25 d/logits 0.25; sl1_b1e-6 loc 0.13 cls 0.25 d/deltas 0.00 d/logits 0.25; sl1_b0.111_w loc 0.25 cls 0.25 d/deltas 0.00 d/logits 0.25; sl1_b1 loc 0.00 cls 0.25 d/deltas 0.03 d/logits 0.25"""
    pre = f"rpn/{kind}"
    A, B, N, *_ = _rpn_inputs(kind, "cpu")
    loss2, dhead = _rpn_run(kind, dev)
    labels = T("rpn/labels")
    got = {"grad_logits": dhead[:, :, :A].reshape(B, N).double(), "grad_deltas": dhead[:, :, A + 1:5 * A + 1].reshape(B, N, 4).double()}
    for i, name in enumerate(("cls", "loc")):
        l64 = float(G[f"{pre}/loss/f64"][i])
        err, bar = abs(float(loss2[i]) - l64), _bar(G[f"{pre}/dev_loss"][i], l64)
        print(f"{pre}: loss_rpn_{name} {float(loss2[i]):.9g} err {err:.3g} bar {bar:.3g} ratio {err / bar:.2f}")
        assert err <= bar, name
    for name, g in got.items():
        g64 = G[f"{pre}/{name}/f64"]
        err, bar = float((g - torch.from_numpy(g64)).abs().max()), _bar(G[f"{pre}/dev_{name}"], np.abs(g64).max())
        print(f"{pre}: {name} err {err:.3g} bar {bar:.3g} ratio {err / bar:.2f}")
        assert err <= bar, name
    assert float(got["grad_logits"][labels == -1].abs().max()) == 0 and float(got["grad_deltas"][labels != 1].abs().max()) == 0
    assert float(got["grad_deltas"][labels == 1].abs().max()) > 0
    assert float(dhead[:, :, A].abs().max()) == 0 and float(dhead[:, :, 5 * A + 1:].abs().max()) == 0
    again = _rpn_run(kind, dev)
    assert torch.equal(again[0], loss2) and torch.equal(again[1], dhead)


@pytest.mark.parametrize("kind", ("giou", "sl1_b0.111_w"))
def test_rpn_kernel_bf16_gradient(dev, kind):
    l32, d32 = _rpn_run(kind, dev)
    l16, d16 = _rpn_run(kind, dev, grad_dtype=torch.bfloat16)
    assert torch.equal(l16, l32)
    _one_bf16_ulp(d16, d32)


def test_rpn_ex_at_smooth_l1_beta_0_is_the_plain_export(dev):
    """(UNIT_BOXLOSS_SMOOTH_L1, 0.0f) through unit_rpn_loss_ex: bit for bit unit_rpn_loss_w, and unit_rpn_loss where the weights are 1"""
    from unit_amd import ops
    for kind in ("sl1_b1e-6", "sl1_b0.111_w"):          # (inputs only: the second has loss weights (0.5, 2))
        A, B, N, head, labels, match, gt, anchors = _rpn_inputs(kind, dev)
        norm, weights = int(G["rpn/batch_size_per_image"]) * B, tuple(float(v) for v in G[f"rpn/{kind}/weights"])
        for dtype in (torch.float32, torch.bfloat16):
            plain = ops.rpn_loss(head, A, A + 1, labels, match, gt, anchors, norm, dtype, weights=weights)
            loss2, dhead = _rpn_run(kind, dev, grad_dtype=dtype, raw=(0, 0.0))
            assert torch.equal(loss2, plain[0].cpu()) and torch.equal(dhead, plain[1].cpu()), (kind, dtype)


# ---------------------------------------------------------------------------------------------------- through the model
def _setup(box=("smooth_l1", 0.0), rpn=("smooth_l1", 0.0), mode="bf16"):
    """tests/test_pcl_model_gpu.py::_setup with the four keys"""
    from unit_amd import config
    from unit_amd.modeling import build_model
    from unit_amd.synthetic import init_synthetic_weights
    cfg = config.voc_rcnn_c4_split1(50)
    cfg.MODEL.DEVICE = "cuda"
    cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = 32
    cfg.MODEL.RPN.PRE_NMS_TOPK_TRAIN, cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN = 600, 100
    cfg.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR.TYPE = "PCL"
    cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE, cfg.MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA = box
    cfg.MODEL.RPN.BBOX_REG_LOSS_TYPE, cfg.MODEL.RPN.SMOOTH_L1_BETA = rpn
    cfg.SOLVER.WARMUP_ITERS = 4
    cfg.SEED = 3
    model = build_model(cfg)
    init_synthetic_weights(model, seed=1)
    model.train()
    model.compute_mode = mode
    return cfg, model


class _Spy:
    """records what the fused step hands to the two loss calls, and what they return"""

    def __init__(self, model, monkeypatch):
        from unit_amd import ops
        self.box, self.rpn = {}, {}
        bp = model.roi_heads.box_predictor
        inner_box, inner_rpn = bp.sup_losses, ops.rpn_loss

        def sup_losses(lin_sup, lin_sup_weak, roi_cls, rois5, roi_gt, loss_out, grad_dtype):
            dy, scores = inner_box(lin_sup, lin_sup_weak, roi_cls, rois5, roi_gt, loss_out, grad_dtype)
            self.box.update(lin_sup=lin_sup, roi_cls=roi_cls, rois5=rois5, roi_gt=roi_gt, dy=dy)
            return dy, scores

        def rpn_loss(*a, **k):
            out = inner_rpn(*a, **k)
            self.rpn.update(args=a, kwargs=dict(k), loss2=out[0], dhead=out[1])
            return out
        monkeypatch.setattr(bp, "sup_losses", sup_losses, raising=False)
        monkeypatch.setattr(ops, "rpn_loss", rpn_loss)


def _fused_step(box, rpn, monkeypatch, mode="bf16"):
    from unit_amd.modeling.rcnn import LOSS_NAMES
    from unit_amd.synthetic import synthetic_batch
    cfg, model = _setup(box, rpn, mode)
    spy = _Spy(model, monkeypatch)
    batch = model.pack_batch(*synthetic_batch(2, 2, hw=(128, 192), seed=50, max_gt=4))
    step = model.forward_train(batch, early_backward=True)
    model.backward_train(step)
    torch.cuda.synchronize()
    monkeypatch.undo()
    return model, spy, dict(zip(LOSS_NAMES, step.losses.clone()))


def _by_hand(model, spy, box, rpn):
    """the two loss kernels called by hand on the step's own tensors -> (loss_box_reg, dy block, loss2, dhead)"""
    from unit_amd import ops
    bp, s = model.roi_heads.box_predictor, spy.box
    k = bp.num_classes
    dy = torch.zeros_like(s["dy"])
    lb = ops.box_reg_loss(s["lin_sup"], bp.col_bbox, k, s["roi_cls"], s["rois5"], s["roi_gt"], bp.bbox_reg_weights, dy=dy, dcol0=bp.col_bbox,
                          loss_type=box[0], beta=box[1])
    kw = {k_: v for k_, v in spy.rpn["kwargs"].items() if k_ not in ("loss_out", "loss_type", "beta")}
    loss2, dhead = ops.rpn_loss(*spy.rpn["args"], loss_type=rpn[0], beta=rpn[1], **kw)
    return lb[0], dy[:, bp.col_bbox:bp.col_bbox + 4 * k], loss2, dhead


@pytest.mark.parametrize("box,rpn", [(("giou", 0.0), ("giou", 0.0)), (("smooth_l1", 1.0 / 9), ("smooth_l1", 1.0 / 9))])
def test_fused_step_beside_the_default_step_and_by_hand(dev, monkeypatch, box, rpn):
    """every loss but loss_box_reg and loss_rpn_loc is bit-equal to the default step's; those two are finite, different, and -- with the
    gradients dy / dhead -- what the _ex kernels give when called by hand on the step's own tensors"""
    _, _, l0 = _fused_step(("smooth_l1", 0.0), ("smooth_l1", 0.0), monkeypatch)
    m1, spy, l1 = _fused_step(box, rpn, monkeypatch)
    for name in l0:
        if name in ("loss_box_reg", "loss_rpn_loc"):
            assert torch.isfinite(l1[name]) and float(l1[name]) > 0 and not torch.equal(l0[name], l1[name]), (name, l0[name], l1[name])
        else:
            assert torch.equal(l0[name], l1[name]), (name, l0[name], l1[name])
    assert spy.rpn["kwargs"]["loss_type"] == rpn[0] and spy.rpn["kwargs"]["beta"] == rpn[1]
    lb, dyb, loss2, dhead = _by_hand(m1, spy, box, rpn)
    bp = m1.roi_heads.box_predictor
    assert torch.equal(lb, l1["loss_box_reg"]) and torch.equal(loss2[1], l1["loss_rpn_loc"]) and torch.equal(loss2[0], l1["loss_rpn_cls"])
    assert float(dyb.float().abs().max()) > 0 and torch.equal(dyb, spy.box["dy"][:, bp.col_bbox:bp.col_bbox + 4 * bp.num_classes])
    assert float(dhead.float().abs().max()) > 0 and torch.equal(dhead, spy.rpn["dhead"])
    # ... and not what the default kernels give on the same tensors
    lb0, _, loss20, _ = _by_hand(m1, spy, ("smooth_l1", 0.0), ("smooth_l1", 0.0))
    assert not torch.equal(lb0, lb) and not torch.equal(loss20[1], loss2[1])


def test_module_level_training_gives_the_fused_steps_losses_and_gradients(dev):
    """backbone -> WSRPN.forward -> WSROIHeadNoMeta.forward in training mode with GIoU on both heads, sum(losses).backward(): the losses()
    of the two modules carry a graph (train_modules._RpnFn, the ROI node) and reproduce the fused step on the same weights, images and
    permutations -- the eight losses to 1e-6 (fp32), the gradients of the two regression layers to 1e-5 of their largest entry"""
    from unit_amd.modeling import build_model
    from unit_amd.modeling.rcnn import LOSS_NAMES
    from unit_amd.structures import ImageList
    from unit_amd.synthetic import synthetic_batch
    giou = ("giou", 0.0)
    cfg, ref_model = _setup(giou, giou, mode="fp32")
    ref_model.compute_dtype = torch.float32
    hw = (128, 192)
    sup, weak = synthetic_batch(2, 2, hw=hw, seed=5, max_gt=4)
    batch = ref_model.pack_batch(sup, weak)
    ref_model._ensure_ready()
    perms = ref_model.sampling_permutations(2, 8 * 12 * 15, cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN + batch.gt_boxes.shape[1])
    step = ref_model.forward_train(batch, perms, early_backward=True)
    ref_model.backward_train(step)
    ref_losses = dict(zip(LOSS_NAMES, step.losses.cpu().tolist()))
    ref_grads = {n: q.grad.detach().clone() for n, q in ref_model.named_parameters() if q.requires_grad}
    model = build_model(cfg)
    model.load_state_dict(ref_model.state_dict())
    model.train()
    for m in model.modules():
        m.compute_dtype = torch.float32
    assert model.proposal_generator.box_reg_loss_type == "giou" and model.roi_heads.box_predictor.box_reg_loss_type == "giou"
    mean = torch.tensor(cfg.MODEL.PIXEL_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(cfg.MODEL.PIXEL_STD).view(1, 3, 1, 1)
    pre = lambda items: ((torch.stack([x["image"] for x in items]) - mean) / std).to(dev)
    images, weak_images = ImageList(None, [hw, hw]), ImageList(None, [hw, hw])
    gt = [x["instances"] for x in sup]
    features, weak_features = model.backbone(pre(sup)), model.backbone(pre(weak))
    model.proposal_generator.next_perm = perms["rpn"]
    proposals, proposal_losses = model.proposal_generator(images, features, gt)
    with torch.no_grad():
        weak_proposals, _ = model.proposal_generator(weak_images, weak_features, None)
    model.roi_heads.next_perm = perms["roi"]
    _, detector_losses = model.roi_heads(images, features, proposals, gt, weak_images=weak_images, weak_features=weak_features,
                                         weak_proposals=weak_proposals, weak_targets=[x["instances"].gt_classes for x in weak])
    losses = dict(detector_losses)
    losses.update(proposal_losses)
    assert set(losses) == set(LOSS_NAMES[:8])
    sum(losses.values()).backward()
    for k, v in losses.items():
        assert abs(float(v) - ref_losses[k]) <= 1e-6 * max(1.0, abs(ref_losses[k])), (k, float(v), ref_losses[k])
    params = dict(model.named_parameters())
    for n in ("roi_heads.box_predictor.bbox_pred_delta.weight", "proposal_generator.rpn_head.anchor_deltas.weight"):
        g, gr = params[n].grad.detach(), ref_grads[n]
        assert float(gr.abs().max()) > 0 and float((g - gr).abs().max()) <= 1e-5 * float(gr.abs().max()) + 1e-8, n


def test_predictor_losses_with_a_graph_are_the_kernels(dev):
    """SupervisedDetectorOutputsBase.losses on predictions that require grad (train_modules._SupLossFn): loss_box_reg and d/d(bbox), at any
    loss weight, are unit_box_reg_loss_ex's loss and dy; without a graph the same value"""
    from unit_amd import config, ops
    from unit_amd.modeling.fast_rcnn import SupervisedDetectorOutputsBase
    from unit_amd.structures import Boxes, Instances, ShapeSpec
    shape, K = "K20_R65", 20
    for kind in ("giou", "sl1_b0.111"):
        cfg = config.get_cfg()
        cfg.MODEL.ROI_HEADS.NUM_CLASSES = K
        cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE, cfg.MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA = _type_of(kind), float(G[f"box/{shape}/{kind}/beta"])
        bp = SupervisedDetectorOutputsBase(cfg, ShapeSpec(channels=128)).to(dev)
        bp.train()
        labels = T(f"box/{shape}/labels")
        keep = labels >= 0          # an Instances list has no empty slots
        _, _, col0, _, _, bbox, _, rois5, gt = _box_inputs(shape, kind, dev)
        bb = bbox[keep.to(dev), col0:col0 + 4 * K].contiguous().requires_grad_(True)
        sc = torch.zeros(int(keep.sum()), K + 1, device=dev, requires_grad=True)
        gc = labels[keep].to(dev)
        props = [Instances((480, 640), proposal_boxes=Boxes(rois5[keep.to(dev), 1:]), gt_boxes=Boxes(gt[keep.to(dev)]), gt_classes=gc.long())]
        out = bp.losses([sc, bb], props)
        (out["loss_cls"] + 3.0 * out["loss_box_reg"]).backward()
        dy = torch.zeros_like(bb)
        r5 = torch.cat([torch.zeros(len(gc), 1, device=dev), rois5[keep.to(dev), 1:]], 1)
        want = ops.box_reg_loss(bb.detach(), 0, K, gc.int(), r5, gt[keep.to(dev)].contiguous(), BOX_WEIGHTS, dy=dy, loss_type=bp.box_reg_loss_type,
                                beta=bp.smooth_l1_beta)
        assert torch.equal(out["loss_box_reg"].detach(), want[0]) and float(dy.abs().max()) > 0 and torch.equal(bb.grad, dy * 3.0)
        with torch.no_grad():
            assert torch.equal(bp.losses([sc.detach(), bb.detach()], props)["loss_box_reg"], want[0])
        l64 = float(G[f"box/{shape}/{kind}/loss/f64"])
        assert abs(float(want[0]) - l64) <= _bar(G[f"box/{shape}/{kind}/dev_loss"], l64)


def _meta_ops():
    """the operators tools/stock_ops.py counts as pure metadata / allocation (read from that file: one list)"""
    with open(os.path.join(ROOT, "tools", "stock_ops.py")) as f:
        m = re.search(r"^META = (\{.*?\})", f.read(), flags=re.S | re.M)
    return ast.literal_eval(m.group(1))


def _six_steps(box, rpn, log_step=None):
    """six eager steps and the same six through ReplayedStep(warmup_steps=2) -> (eager losses, replayed losses, m1, m2, rs, logged ATen calls)"""
    from torch.utils._python_dispatch import TorchDispatchMode
    from unit_amd import engine
    from unit_amd.solver import FlatSGD
    from unit_amd.synthetic import synthetic_batch
    data = [synthetic_batch(2, 2, hw=(128, 192), seed=50 + i, max_gt=4) for i in range(3)]
    seq = [data[i] for i in (0, 1, 2, 1, 0, 2)]
    meta = _meta_ops()
    calls = []

    class Log(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            parts = str(func).split(".")
            if (parts[1] if len(parts) >= 2 else parts[0]) not in meta:
                calls.append(str(func))
            return func(*args, **(kwargs or {}))
    cfg, m1 = _setup(box, rpn)
    o1 = FlatSGD(m1, cfg)
    ref = []
    for j, d in enumerate(seq):
        b = m1.pack_batch(*d, gt_buckets=engine.GraphedStep.GT_BUCKETS)
        o1._bind()
        o1.use_device_lr(m1.device)
        log = Log() if j == log_step else None
        if log is not None:
            log.__enter__()
        step = m1.forward_train(b, early_backward=True)
        m1.backward_train(step)
        o1.step()
        if log is not None:
            log.__exit__(None, None, None)
        ref.append(step.losses.clone())
    torch.cuda.synchronize()
    cfg, m2 = _setup(box, rpn)
    rs = engine.ReplayedStep(m2, FlatSGD(m2, cfg), warmup_steps=2)
    got = [rs.run(*d).clone() for d in seq]
    torch.cuda.synchronize()
    return ref, got, m1, m2, rs, calls


def _plan_names(rs):
    plan = next(iter(rs.plans.values()))[0]
    return [n for it in plan.items if it[0] == "calls" for n in it[3]]


def test_replayed_giou_steps_equal_eager_and_launch_no_stock_operator(dev):
    giou = ("giou", 0.0)
    ref, got, m1, m2, rs, calls = _six_steps(giou, giou, log_step=3)
    assert calls == [], calls          # a steady-state step dispatches no stock ATen kernel
    assert rs.stats == {"eager": 2, "captured": 1, "replayed": 3}
    names = _plan_names(rs)
    assert names.count("unit_box_reg_loss_ex") == 1 and names.count("unit_rpn_loss_ex") == 1
    assert "unit_box_reg_loss" not in names and "unit_rpn_loss_w" not in names and "unit_rpn_loss" not in names
    for k, (a, b) in enumerate(zip(got, ref)):
        assert torch.isfinite(a).all() and torch.equal(a, b), (k, a.tolist(), b.tolist())
    assert torch.equal(m2.store.params, m1.store.params)


def test_default_config_replays_the_parent_commits_call_list(dev):
    """with Detectron2's defaults the recorded plan is, name for name and in order, the one the commit before the switch recorded for this very
    _setup, data sequence and ReplayedStep(warmup_steps=2) (tests/golden/box_loss_parent_plan.json, written on that commit)"""
    with open(os.path.join(GDIR, "box_loss_parent_plan.json")) as f:
        parent = json.load(f)
    ref, got, m1, m2, rs, _ = _six_steps(("smooth_l1", 0.0), ("smooth_l1", 0.0))
    names = _plan_names(rs)
    assert len(names) == len(parent["names"]) and names == parent["names"]
    assert "unit_box_reg_loss" in names and "unit_rpn_loss_w" in names and not any(n.endswith("_loss_ex") for n in names)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    # ... and computes what the parent computed: its six loss vectors, bit for bit
    assert [a.tolist() for a in got] == parent["losses"]


def test_giou_step_at_baseline_size(dev, monkeypatch):
    """R101, 600 x 1000, 2 + 2 images, bf16, GIoU on both heads: finite losses, the two box losses equal to the by-hand calls"""
    from unit_amd import config
    from unit_amd.modeling import build_model
    from unit_amd.modeling.rcnn import LOSS_NAMES
    from unit_amd.synthetic import init_synthetic_weights, synthetic_batch
    giou = ("giou", 0.0)
    cfg = config.voc_rcnn_c4_split1(101)
    cfg.MODEL.DEVICE = "cuda:0"
    cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE = cfg.MODEL.RPN.BBOX_REG_LOSS_TYPE = "giou"
    cfg.SEED = 0
    model = build_model(cfg)
    init_synthetic_weights(model, seed=1)
    model.train()
    model.compute_mode = "bf16"
    spy = _Spy(model, monkeypatch)
    batch = model.pack_batch(*synthetic_batch(2, 2, seed=100))
    step = model.forward_train(batch, early_backward=True)
    model.backward_train(step)
    torch.cuda.synchronize()
    monkeypatch.undo()
    losses = dict(zip(LOSS_NAMES, step.losses.clone()))
    assert torch.isfinite(step.losses).all(), losses
    assert spy.box["lin_sup"].shape[0] == 2 * 512 and spy.box["dy"].dtype == torch.bfloat16
    lb, dyb, loss2, dhead = _by_hand(model, spy, giou, giou)
    bp = model.roi_heads.box_predictor
    assert float(lb) > 0 and torch.equal(lb, losses["loss_box_reg"])
    assert float(loss2[1]) > 0 and torch.equal(loss2[1], losses["loss_rpn_loc"]) and torch.equal(loss2[0], losses["loss_rpn_cls"])
    assert torch.equal(dyb, spy.box["dy"][:, bp.col_bbox:bp.col_bbox + 4 * bp.num_classes]) and torch.equal(dhead, spy.rpn["dhead"])
