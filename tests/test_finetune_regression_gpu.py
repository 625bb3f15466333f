"""The second stage on a REGRESSION_BRANCH model, on the device: unit_transfer_predictions_ex on the reference's own Linear outputs, the
fine-tune predictor, the fused / module-level / replayed fine-tune step, the mask fine-tune head, checkpoints and inference, against
tests/golden/finetune_regression_golden.npz (the reference's SupervisedDetectorOutputsFineTune with regression_branch=True).

Tolerances. Kernel: an element fed by three fp32 additions and nothing else -- background, base classes, every column without a similarity --
is torch.equal to the reference's; the novel columns carry a dot product over the base classes: rtol 1e-5 / atol 1e-5, what
test_unit_golden_gpu.py applies to unit_transfer_predictions. Predictor (this project's fp32 GEMM in the path): 1e-4 on values, 1e-4 relative
on losses, rtol 2e-4 / atol 2e-6 on the gradients at the ft heads' outputs, rtol 2e-3 on a weight gradient (test_regression_branch_gpu.py's bars)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GDIR = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GDIR)
G = np.load(os.path.join(GDIR, "finetune_regression_golden.npz"))
TAGS = ("F20", "F80", "F1")
KINDS = {"sl1_b0": ("smooth_l1", 0.0), "sl1_b0.5": ("smooth_l1", 0.5), "giou": ("giou", 0.0)}
JUNK0 = 5          # columns in front of every block that no kernel may read (they hold 7.0)
DPAD = 128         # the Linear kernels are built for the model's feature widths: the fixture's D = 32 features are zero-padded
FROZEN = ["weak_detector_head", "cls_score_delta", "bbox_pred_delta", "embeddings"]
FT_KEYS = ["roi_heads.box_predictor." + n for n in ("cls_score_ft.weight", "cls_score_ft.bias", "bbox_pred_ft.weight", "bbox_pred_ft.bias")]
REG = "roi_heads.box_predictor.weak_detector_head.regression_branch_"


def T(k):
    return torch.from_numpy(G[k])


def _roles(tag, dev):
    K, base, novel = int(G[f"{tag}/K"]), G[f"{tag}/base"].tolist(), G[f"{tag}/novel"].tolist()
    role, slot = torch.zeros(K, dtype=torch.int8), torch.zeros(K, dtype=torch.int32)
    for i, c in enumerate(base):
        role[c], slot[c] = 1, i
    for i, c in enumerate(novel):
        role[c], slot[c] = 2, i
    return dict(base=torch.tensor(base, dtype=torch.int32, device=dev), novel=torch.tensor(novel, dtype=torch.int32, device=dev),
                role=role.to(dev), slot=slot.to(dev))


def _blocks(tag, which, dev):
    """[junk | cls (K + 1) | junk | bbox (4K) | pad to 8] filled with 7.0 outside the two blocks -> (matrix, cls column, bbox column)"""
    K = int(G[f"{tag}/K"])
    c_cls = JUNK0
    c_box = c_cls + K + 1 + JUNK0
    ld = (c_box + 4 * K + 7) // 8 * 8
    m = torch.full((T(f"{tag}/x").shape[0], ld), 7.0)
    m[:, c_cls:c_cls + K + 1], m[:, c_box:c_box + 4 * K] = T(f"{tag}/lin_{which}_cls"), T(f"{tag}/lin_{which}_bbox")
    return m.to(dev), c_cls, c_box


def _sims(tag, mode, dev):
    if mode == "none":
        return None, None
    out = []
    for h in ("cls", "bbox"):
        s = T(f"{tag}/sim_{h}")
        out.append((s[:1].expand_as(s) if mode == "2d" else s).contiguous().to(dev))
    return out


# ---------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("mode", ["3d", "2d", "none"])
@pytest.mark.parametrize("tag", TAGS)
def test_kernel_on_the_references_linear_outputs(dev, tag, mode):
    from unit_amd import ops
    K = int(G[f"{tag}/K"])
    t = _roles(tag, dev)
    lin, c_c, c_b = _blocks(tag, "delta", dev)
    weak, w_c, w_b = _blocks(tag, "weak", dev)
    ft, f_c, f_b = _blocks(tag, "ft", dev)
    sc_, sb_ = _sims(tag, mode, dev)
    call = lambda wb: ops.transfer_predictions(lin, c_c, c_b, K, weak, w_c, 1, sc_, sb_, t["base"], t["novel"], t["role"], t["slot"], ft=ft,
                                               fccol0=f_c, fbcol0=f_b, wbcol0=wb)
    scores, bbox = (v.cpu() for v in call(w_b))
    want_s, want_b = T(f"{tag}/scores_{mode}"), T(f"{tag}/bbox_{mode}")
    base = T(f"{tag}/base").long()
    novel = T(f"{tag}/novel").long()
    cols = torch.cat([base, torch.tensor([K])])
    bcols = (4 * base[:, None] + torch.arange(4)).flatten()
    ncols = (4 * novel[:, None] + torch.arange(4)).flatten()
    print(f"{tag}/{mode}: scores max abs err {float((scores - want_s).abs().max()):.3g}, bbox {float((bbox - want_b).abs().max()):.3g}; "
          f"exact columns differ in {int((scores[:, cols] != want_s[:, cols]).sum())} + {int((bbox[:, bcols] != want_b[:, bcols]).sum())} elements")
    assert torch.equal(scores[:, cols], want_s[:, cols])          # ((delta) + weak) + ft: fails with (o + ft) + weak
    assert torch.equal(bbox[:, bcols], want_b[:, bcols])
    if mode == "none":
        assert torch.equal(scores, want_s) and torch.equal(bbox, want_b)
    torch.testing.assert_close(scores[:, novel], want_s[:, novel], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(bbox[:, ncols], want_b[:, ncols], rtol=1e-5, atol=1e-5)
    # wbcol0 = -1 is the plain entry, bit for bit
    plain = ops.transfer_predictions(lin, c_c, c_b, K, weak, w_c, 1, sc_, sb_, t["base"], t["novel"], t["role"], t["slot"], ft=ft, fccol0=f_c, fbcol0=f_b)
    neg = call(-1)
    assert torch.equal(neg[0], plain[0]) and torch.equal(neg[1], plain[1])
    assert torch.equal(plain[0].cpu(), scores) and not torch.equal(plain[1].cpu(), bbox)          # the scores never knew wbcol0; the deltas do


def test_kernel_argument_checks(dev):
    """R = 0 is OK and launches nothing; a wbcol0 whose 4K columns pass the row stride of `weak`, or one without `weak`, is an error with a
    message, and the output buffers keep what they held"""
    from unit_amd import _lib, ops
    tag, K = "F20", 20
    t = _roles(tag, dev)
    lin, c_c, c_b = _blocks(tag, "delta", dev)
    weak, w_c, w_b = _blocks(tag, "weak", dev)
    ft, f_c, f_b = _blocks(tag, "ft", dev)
    s0, b0 = ops.transfer_predictions(lin[:0], c_c, c_b, K, weak[:0], w_c, 1, None, None, t["base"], t["novel"], t["role"], t["slot"], ft=ft[:0],
                                      fccol0=f_c, fbcol0=f_b, wbcol0=w_b)
    assert s0.shape == (0, K + 1) and b0.shape == (0, 4 * K)
    ldw = weak.shape[1]
    with pytest.raises(_lib.UnitLibError, match="transfer_predictions_ex.*row stride"):
        ops.transfer_predictions(lin, c_c, c_b, K, weak, w_c, 1, None, None, t["base"], t["novel"], t["role"], t["slot"], ft=ft, fccol0=f_c,
                                 fbcol0=f_b, wbcol0=ldw - 4 * K + 1)
    with pytest.raises(_lib.UnitLibError, match="transfer_predictions_ex.*NULL"):
        ops.transfer_predictions(lin, c_c, c_b, K, None, 0, 1, None, None, t["base"], t["novel"], t["role"], t["slot"], ft=ft, fccol0=f_c,
                                 fbcol0=f_b, wbcol0=0)
    r = lin.shape[0]
    scores, bbox = torch.full((r, K + 1), 3.0, device=dev), torch.full((r, 4 * K), 3.0, device=dev)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    st = _lib.lib().unit_transfer_predictions_ex(p(lin), lin.shape[1], c_c, c_b, K, p(weak), ldw, w_c, 1, ldw, p(ft), ft.shape[1], f_c, f_b, None, None,
                                                 p(t["base"]), 15, p(t["novel"]), 5, p(t["role"]), p(t["slot"]), p(scores), K + 1, p(bbox), 4 * K, r,
                                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st != 0 and b"row stride" in _lib.lib().unit_last_error()
    assert float((scores - 3.0).abs().max()) == 0.0 and float((bbox - 3.0).abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------- 2. the predictor
def _predictor(tag, dev, cls_name="SupervisedDetectorOutputsFineTune", zero_ft=False):
    from unit_amd import config
    from unit_amd.layers import invalidate_prepared
    from unit_amd.modeling import fast_rcnn
    from unit_amd.structures import ShapeSpec
    K = int(G[f"{tag}/K"])
    cfg = config.get_cfg()
    cfg.MODEL.ROI_HEADS.NUM_CLASSES = K
    cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = 0.05
    cfg.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR.REGRESSION_BRANCH = True
    cfg.MODEL.FREEZE_LAYERS.FAST_RCNN = list(FROZEN)
    cfg.DATASETS.FEWSHOT.BASE_CLASSES_ID, cfg.DATASETS.FEWSHOT.NOVEL_CLASSES_ID = G[f"{tag}/base"].tolist(), G[f"{tag}/novel"].tolist()
    bp = getattr(fast_rcnn, cls_name)(cfg, ShapeSpec(channels=DPAD))
    assert float(bp.bbox_pred_delta.weight.detach().abs().max()) == 0.0          # fast_rcnn.py:322-323 under the switch, FineTune as Base
    bp = bp.to(dev)
    named = dict(bp.named_parameters())
    with torch.no_grad():
        for k in G.files:
            if k.startswith(f"{tag}/param/") and k[len(f"{tag}/param/"):] in named:
                p, w = named[k[len(f"{tag}/param/"):]], T(k).to(dev)
                p.zero_()
                p[..., :w.shape[-1]].copy_(w) if w.dim() > 1 else p.copy_(w)
        if zero_ft and hasattr(bp, "cls_score_ft"):
            for l in (bp.cls_score_ft, bp.bbox_pred_ft):
                l.weight.zero_(), l.bias.zero_()
    for m in bp.modules():
        m.compute_dtype = torch.float32
    invalidate_prepared()
    pad = lambda t: torch.cat([t, torch.zeros(t.shape[0], DPAD - t.shape[1])], 1).to(dev)
    return bp, pad(T(f"{tag}/x")), pad(T(f"{tag}/xw"))


def _proposals(tag, dev):
    from unit_amd.structures import Boxes, Instances
    sizes = G[f"{tag}/sizes"].tolist()
    off = np.insert(np.cumsum(sizes), 0, 0)
    return [Instances((300, 400), proposal_boxes=Boxes(T(f"{tag}/prop_boxes")[off[i]:off[i + 1]].to(dev)),
                      gt_boxes=Boxes(T(f"{tag}/prop_gt_boxes")[off[i]:off[i + 1]].to(dev)),
                      gt_classes=T(f"{tag}/prop_gt_classes")[off[i]:off[i + 1]].long().to(dev)) for i in range(len(sizes))]


@pytest.mark.parametrize("tag", TAGS)
def test_predictor_against_the_reference(dev, tag):
    """SupervisedDetectorOutputsFineTune under the switch: forward in training (with a graph) and in eval for a 3-D, a 2-D and no similarity,
    both losses for the three box-loss kinds, the gradients at the ft heads' outputs, a weight gradient, and where no gradient may arrive"""
    bp, x, xw = _predictor(tag, dev)
    nov_t, base_t = T(f"{tag}/novel").long(), T(f"{tag}/base").long()
    props = _proposals(tag, dev)
    sim3 = {"cls": T(f"{tag}/sim_cls").to(dev), "bbox": T(f"{tag}/sim_bbox").to(dev)}
    sim2 = {k: v[0].contiguous() for k, v in sim3.items()}
    fwd = lambda xin, sim: bp(xin, nov_t, base_t, supervised_branch_x_weak=xw, x_weak=None, similarity=sim)
    for nm, sim in (("3d", sim3), ("2d", sim2), ("none", None)):
        bp.train()
        (st, bt), weak_ret = fwd(x.clone().requires_grad_(True), sim)
        assert weak_ret is None and st.requires_grad and bt.requires_grad
        with torch.no_grad():          # values under no_grad: the same kernels, the same bits
            (sn, bn), _ = fwd(x, sim)
        assert torch.equal(sn, st.detach()) and torch.equal(bn, bt.detach())
        bp.eval()
        (se, be), _ = fwd(x, sim)
        assert not se.requires_grad and torch.equal(se, sn) and torch.equal(be, bn)
        print(f"{tag}/{nm}: scores err {float((sn.cpu() - T(f'{tag}/scores_{nm}')).abs().max()):.3g} bbox err {float((bn.cpu() - T(f'{tag}/bbox_{nm}')).abs().max()):.3g}")
        for got in (st.detach(), se):
            torch.testing.assert_close(got.cpu(), T(f"{tag}/scores_{nm}"), rtol=1e-4, atol=1e-4)
        for got in (bt.detach(), be):
            torch.testing.assert_close(got.cpu(), T(f"{tag}/bbox_{nm}"), rtol=1e-4, atol=1e-4)
    assert bool(torch.isfinite(se).all())          # no novel column is filled with -inf
    bp.train()
    for kind, (loss_type, beta) in KINDS.items():
        bp.box_reg_loss_type, bp.smooth_l1_beta = loss_type, beta
        for p in bp.parameters():
            p.grad = None
        xg = x.clone().requires_grad_(True)
        (scores, bbox), _ = fwd(xg, sim3)
        scores.retain_grad(), bbox.retain_grad()
        losses = bp.losses([scores, bbox], props)
        assert set(losses) == {"loss_cls", "loss_box_reg"}
        for k, want in (("loss_cls", float(G[f"{tag}/loss_cls"])), ("loss_box_reg", float(G[f"{tag}/{kind}/loss_box_reg"]))):
            got = float(losses[k].detach())
            print(f"{tag}/{kind} {k}: {got:.8g} vs {want:.8g}")
            assert abs(got - want) <= 1e-4 * max(1.0, abs(want)), (k, got, want)
        sum(losses.values()).backward()
        torch.testing.assert_close(scores.grad.cpu(), T(f"{tag}/grad_cls_ft_out"), rtol=2e-4, atol=2e-6)
        torch.testing.assert_close(bbox.grad.cpu(), T(f"{tag}/{kind}/grad_bbox_ft_out"), rtol=2e-4, atol=2e-6)
        want_gw = T(f"{tag}/grad_cls_ft_out").t() @ T(f"{tag}/x")
        torch.testing.assert_close(bp.cls_score_ft.weight.grad.cpu()[:, :32], want_gw, rtol=2e-3, atol=2e-5 * float(want_gw.abs().max()))
        assert float(bp.bbox_pred_ft.weight.grad.abs().max()) > 0 and xg.grad is not None
        for n, p in bp.named_parameters():
            if n.split(".")[0] in ("weak_detector_head", "cls_score_delta", "bbox_pred_delta"):
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
        with torch.no_grad():
            l_ng = bp.losses([scores.detach(), bbox.detach()], props)
        assert all(torch.equal(l_ng[k], losses[k].detach()) for k in l_ng)
    bp.box_reg_loss_type, bp.smooth_l1_beta = "smooth_l1", 0.0
    bp.eval()
    (se, be), _ = fwd(x, sim3)
    res, inds = bp.inference([se, be], props)
    assert len(res) == len(props) and sum(len(r) for r in res) > 0
    with pytest.raises(NotImplementedError):
        bp.inference([se, be], props, tta=True)
    with pytest.raises(NotImplementedError):
        bp(None, nov_t, base_t, x_weak=xw)


@pytest.mark.parametrize("tag", ["F20", "F80"])
def test_zeroed_ft_heads_are_the_base_predictors_eval_forward(dev, tag):
    """ties the new path to the one regression_branch_golden.npz pins: with the ft heads zeroed, the TRAINING forward of the FineTune predictor
    (one launch, unit_transfer_predictions_ex) is torch.equal to the EVAL forward of the Base predictor with the switch (unit_transfer_predictions
    followed by add_weak_deltas) on the same state and similarity"""
    ft, x, xw = _predictor(tag, dev, zero_ft=True)
    base, _, _ = _predictor(tag, dev, "SupervisedDetectorOutputsBase")
    nov_t, base_t = T(f"{tag}/novel").long(), T(f"{tag}/base").long()
    sim3 = {"cls": T(f"{tag}/sim_cls").to(dev), "bbox": T(f"{tag}/sim_bbox").to(dev)}
    sim2 = {k: v[0].contiguous() for k, v in sim3.items()}
    ft.train(), base.eval()
    for sim in (sim3, sim2):
        (s0, b0), _ = ft(x.clone().requires_grad_(True), nov_t, base_t, supervised_branch_x_weak=xw, similarity=sim)
        (s1, b1), _ = base(x, nov_t, base_t, supervised_branch_x_weak=xw, similarity=sim)
        assert torch.equal(s0.detach(), s1) and torch.equal(b0.detach(), b1)


# ---------------------------------------------------------------------------------------------------- 3. the step
HW = (128, 160)


def _setup(on, seed=3, name="voc"):
    from unit_amd import config
    from unit_amd.modeling import build_model
    from unit_amd.synthetic import init_synthetic_weights
    cfg = config.voc_rcnn_c4_split1_ft(50) if name == "voc" else config.coco_rcnn_c4_split1_segm_ft(50)
    cfg.MODEL.DEVICE = "cuda"
    cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE = 32
    cfg.MODEL.RPN.PRE_NMS_TOPK_TRAIN, cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN = 600, 100
    cfg.MODEL.RPN.PRE_NMS_TOPK_TEST, cfg.MODEL.RPN.POST_NMS_TOPK_TEST = 300, 60
    cfg.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR.REGRESSION_BRANCH = on
    ft = cfg.MODEL.ROI_HEADS.FINETUNE_TERMS
    ft.CLASSIFIER, ft.BBOX, ft.MASK = ["lingual"], ["lingual"], ["lingual"]
    cfg.SEED = seed
    model = build_model(cfg)
    init_synthetic_weights(model, seed=1)
    model.train()
    model.compute_mode = "fp32"
    return cfg, model


def _data(k=20, with_masks=False):
    """two steps' worth of two supervised 128 x 160 images whose gt holds novel classes"""
    from unit_amd.synthetic import synthetic_batch
    data = [synthetic_batch(2, 0, hw=HW, seed=80 + i, max_gt=3, num_classes=k, base_ids=list(range(k)))[0] for i in range(2)]
    if with_masks:
        import gen_ref_step as grs
        for sup in data:
            grs.ellipse_masks(sup, HW)
    return data


def _has_novel(cfg, data):
    novel = set(cfg.DATASETS.FEWSHOT.NOVEL_CLASSES_ID)
    return all(any(int(c) in novel for s in sup for c in s["instances"].gt_classes) for sup in data)


def _meta_ops():
    """the operators tools/stock_ops.py counts as pure metadata / allocation (read from that file: one list)"""
    import ast
    import re
    with open(os.path.join(ROOT, "tools", "stock_ops.py")) as f:
        m = re.search(r"^META = (\{.*?\})", f.read(), flags=re.S | re.M)
    return ast.literal_eval(m.group(1))


def _plan_names(rs):
    plan = next(iter(rs.plans.values()))[0]
    return [n for it in plan.items if it[0] == "calls" for n in it[3]]


def test_trainer_finetune_steps_move_the_ft_heads_only(dev):
    """TrainerFineTune.run_step twice: finite losses, the two regression slots stay unused zeros (no weak batch), cls_score_ft / bbox_pred_ft
    move and no other parameter does -- the four frozen regression_branch_* tensors included"""
    from unit_amd import engine
    cfg, m = _setup(True)
    data = _data()
    assert _has_novel(cfg, data)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    tr = engine.TrainerFineTune(cfg, m)
    for sup in data:
        tr.run_step(sup, None)
        ld = tr.loss_dict()
        assert list(ld) == m.loss_names and len(ld) == 11 and all(np.isfinite(v) for v in ld.values()), ld
        assert ld["loss_cls"] > 0 and ld["loss_box_reg"] > 0 and ld["loss_regression_cls"] == 0.0 and ld["loss_regression_bbox"] == 0.0
        assert ld["loss_im_cls"] == 0.0 and ld["loss_oicr_1"] == 0.0
    print({k: round(v, 6) for k, v in ld.items()})
    moved = sorted(n for n, p in m.named_parameters() if float((p.detach() - before[n]).abs().max()) > 0)
    assert moved == sorted(FT_KEYS), moved
    assert all((REG + s) in before for s in ("cls.weight", "bbox.weight"))


def test_fused_step_against_the_module_level_heads(dev):
    """the fused fine-tune step (rcnn.forward_train) and backbone -> WSRPN -> WSROIHeadFineTune.forward in training (train_modules._HeadsFn) on
    the same weights, images and permutations: loss_cls and loss_box_reg agree to 1e-6 relative (fp32), both through the one-launch form"""
    from unit_amd.modeling import build_model
    from unit_amd.structures import ImageList
    cfg, ref_model = _setup(True)
    ref_model.compute_dtype = torch.float32
    with torch.no_grad():          # non-zero ft heads: their forward contribution is in the losses
        g = torch.Generator().manual_seed(9)
        bp = ref_model.roi_heads.box_predictor
        bp.cls_score_ft.weight.copy_((torch.randn(bp.cls_score_ft.weight.shape, generator=g) * 0.01).to(dev))
        bp.bbox_pred_ft.weight.copy_((torch.randn(bp.bbox_pred_ft.weight.shape, generator=g) * 0.001).to(dev))
    sup = _data()[0]
    batch = ref_model.pack_batch(sup, None)
    ref_model._ensure_ready()
    perms = ref_model.sampling_permutations(2, (HW[0] // 16) * (HW[1] // 16) * 15, cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN + batch.gt_boxes.shape[1])
    ref_model.next_perms = perms
    whole = ref_model(batch)
    assert {"loss_cls", "loss_box_reg"} <= set(whole) and not any("regression" in k or "oicr" in k for k in whole)          # (no weak batch)
    assert all(torch.isfinite(v) for v in whole.values())
    sum(whole.values()).backward()
    model = build_model(cfg)
    model.load_state_dict(ref_model.state_dict())
    model.train()
    for m in model.modules():
        m.compute_dtype = torch.float32
    mean, std = torch.tensor(cfg.MODEL.PIXEL_MEAN).view(1, 3, 1, 1), torch.tensor(cfg.MODEL.PIXEL_STD).view(1, 3, 1, 1)
    x = ((torch.stack([s["image"] for s in sup]) - mean) / std).to(dev)
    images, gt = ImageList(None, [HW] * len(sup)), [s["instances"] for s in sup]
    features = model.backbone(x)
    model.proposal_generator.next_perm = perms["rpn"]
    proposals, _ = model.proposal_generator(images, features, gt)
    model.roi_heads.next_perm = perms["roi"]
    _, losses = model.roi_heads(images, features, proposals, gt)
    assert set(losses) == {"loss_cls", "loss_box_reg"}
    for k, v in losses.items():
        got, want = float(v.detach()), float(whole[k].detach())
        print(f"{k}: module {got:.8g} fused {want:.8g}")
        assert v.requires_grad and abs(got - want) <= 1e-6 * max(1.0, abs(want)), (k, got, want)
    sum(losses.values()).backward()
    a, b = model.roi_heads.box_predictor, ref_model.roi_heads.box_predictor
    for l2, l1 in ((a.cls_score_ft, b.cls_score_ft), (a.bbox_pred_ft, b.bbox_pred_ft)):
        assert float((l2.weight.grad - l1.weight.grad).abs().max()) <= 1e-5 * float(l1.weight.grad.abs().max())


def test_replayed_finetune_step_and_its_call_list(dev):
    """four steps eager against four through ReplayedStep: bit-equal losses and parameters; the steady-state step dispatches no stock ATen
    kernel; the recorded list names unit_transfer_predictions_ex once and neither unit_transfer_predictions nor unit_sup_scores, and has
    exactly as many entries as the same configuration records with the switch off, whose list names no _ex entry"""
    from torch.utils._python_dispatch import TorchDispatchMode
    from unit_amd import engine
    from unit_amd.solver import FlatSGD
    data = _data()
    seq = [data[0], data[1], data[0], data[1]]
    cfg, m2 = _setup(True)
    o2 = FlatSGD(m2, cfg)
    ref, stock = [], []
    meta = _meta_ops()

    class Log(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            parts = str(func).split(".")
            if (parts[1] if len(parts) >= 2 else parts[0]) not in meta:
                stock.append(str(func))
            return func(*args, **(kwargs or {}))
    for j, sup in enumerate(seq):
        b = m2.pack_batch(sup, None, gt_buckets=engine.GraphedStep.GT_BUCKETS)
        o2._bind()
        o2.use_device_lr(m2.device)
        log = Log() if j == 3 else None
        if log is not None:
            log.__enter__()
        step = m2.forward_train(b, early_backward=True)
        m2.backward_train(step)
        o2.step()
        if log is not None:
            log.__exit__(None, None, None)
        ref.append(step.losses.clone())
    torch.cuda.synchronize()
    assert stock == [], stock
    cfg, m3 = _setup(True)
    rs = engine.ReplayedStep(m3, FlatSGD(m3, cfg), warmup_steps=1)
    got = [rs.run(sup, None).clone() for sup in seq]
    torch.cuda.synchronize()
    assert rs.stats == {"eager": 1, "captured": 1, "replayed": 2}
    for k, (a, b) in enumerate(zip(got, ref)):
        assert a.numel() == 11 and torch.isfinite(a).all() and torch.equal(a, b), (k, a.tolist(), b.tolist())
    assert torch.equal(m3.store.params, m2.store.params)
    on = _plan_names(rs)
    assert on.count("unit_transfer_predictions_ex") == 1 and "unit_transfer_predictions" not in on and "unit_sup_scores" not in on
    cfg, m4 = _setup(False)
    rs_off = engine.ReplayedStep(m4, FlatSGD(m4, cfg), warmup_steps=1)
    out = [rs_off.run(sup, None) for sup in seq[:2]]
    torch.cuda.synchronize()
    off = _plan_names(rs_off)
    assert out[-1].numel() == 9 and off.count("unit_transfer_predictions") == 1 and "unit_transfer_predictions_ex" not in off
    print(f"recorded entries: switch on {len(on)}, switch off {len(off)}")
    assert len(on) == len(off) > 100          # the switch costs the fine-tune step no launch
    assert [n for n in on if n != "unit_transfer_predictions_ex"] == [n for n in off if n != "unit_transfer_predictions"]


# ---------------------------------------------------------------------------------------------------- 4. the mask fine-tune head
def test_mask_finetune_step_runs_eagerly(dev, monkeypatch):
    """one eager step of the COCO segm fine-tune configuration (K = 80, the box head trains) with the switch on: finite losses incl. loss_mask,
    a gradient on the box head; the similarity is static under the switch, so similarity_backward hands zeros to the weak head's logits --
    the regression columns are never read as a per-RoI term; ReplayedStep refuses the configuration with its present message"""
    from unit_amd import engine
    from unit_amd.modeling import inference
    from unit_amd.modeling.rcnn import LOSS_NAMES
    from unit_amd.solver import FlatSGD
    cfg, m = _setup(True, name="coco")
    sup = _data(80, with_masks=True)[0]
    assert _has_novel(cfg, [sup])
    seen = []
    orig = inference.similarity_backward

    def spy(*a, **k):
        out = orig(*a, **k)
        seen.append(out)
        return out
    monkeypatch.setattr(inference, "similarity_backward", spy)
    batch = m.pack_batch(sup, None)
    m._ensure_ready()
    step = m.forward_train(batch, early_backward=True)
    m.backward_train(step)
    torch.cuda.synchronize()
    ld = dict(zip(m.loss_names, step.losses.cpu().tolist()))
    print({k: round(v, 6) for k, v in ld.items()})
    assert len(ld) == len(LOSS_NAMES) + 2 and all(np.isfinite(v) for v in ld.values())
    assert ld["loss_mask"] > 0 and ld["loss_cls"] > 0 and ld["loss_box_reg"] > 0
    g = dict(m.named_parameters())["roi_heads.box_head.res5.0.conv1.weight"].grad
    assert g is not None and float(g.abs().max()) > 0
    assert len(seen) == 1 and float(seen[0].float().abs().max()) == 0.0
    with pytest.raises(NotImplementedError, match="fine-tune step whose box head trains.*stock torch operators"):
        engine.ReplayedStep(m, FlatSGD(m, cfg), warmup_steps=1)


# ---------------------------------------------------------------------------------------------------- 5. checkpoint and eval
def _detections(model, inp):
    from unit_amd.layers import invalidate_prepared
    invalidate_prepared()
    return model.inference(inp, do_postprocess=False)


def _moved(a, b):
    out = False
    for x, y in zip(a, b):
        n = min(len(x), len(y))
        out |= len(x) != len(y) or float((x.pred_boxes.tensor[:n] - y.pred_boxes.tensor[:n]).abs().max()) > 1e-2
    return out


def test_checkpoints_and_eval(dev):
    """a state dict with the regression_branch_* and the *_ft keys loads with nothing missing and nothing unexpected; a stage-1 state dict of a
    switch-on model loads with exactly the four *_ft tensors missing, left at zero; model.inference returns detections that move when only
    bbox_pred_ft changes and again when only regression_branch_bbox changes"""
    from unit_amd import checkpoint, config
    from unit_amd.modeling import build_model
    from unit_amd.synthetic import init_synthetic_weights, synthetic_batch
    cfg, src = _setup(True)
    g = torch.Generator().manual_seed(11)
    bp = src.roi_heads.box_predictor
    wh = bp.weak_detector_head
    with torch.no_grad():
        for l, s in ((wh.regression_branch_bbox, 0.02), (wh.regression_branch_cls, 0.02), (bp.cls_score_ft, 0.01), (bp.bbox_pred_ft, 0.01)):
            l.weight.copy_((torch.randn(l.weight.shape, generator=g) * s).to(dev))
    state = {k: v.detach().cpu().clone() for k, v in src.state_dict().items()}
    cfg, model = _setup(True, seed=4)
    rep = checkpoint.load_checkpoint(model, state)
    assert rep["missing"] == [] and rep["unexpected"] == []
    assert all(torch.equal(model.state_dict()[k].cpu(), state[k]) for k in FT_KEYS + [REG + "bbox.weight", REG + "cls.bias"])
    # stage 1 of a switch-on model -> the fine-tune model
    c1 = config.voc_rcnn_c4_split1(50)
    c1.MODEL.DEVICE = "cuda"
    c1.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR.REGRESSION_BRANCH = True
    ft = c1.MODEL.ROI_HEADS.FINETUNE_TERMS
    ft.CLASSIFIER, ft.BBOX, ft.MASK = ["lingual"], ["lingual"], ["lingual"]
    s1 = init_synthetic_weights(build_model(c1), seed=2)
    stage1 = {k: v.detach().cpu().clone() for k, v in s1.state_dict().items()}
    assert not any("_ft." in k for k in stage1)
    cfg, fresh = _setup(True, seed=5)
    with torch.no_grad():          # (init_synthetic_weights leaves the ft heads at zero, as the constructor does)
        assert all(float(fresh.state_dict()[k].abs().max()) == 0.0 for k in FT_KEYS)
    rep = checkpoint.load_checkpoint(fresh, stage1)
    assert sorted(rep["missing"]) == sorted(FT_KEYS) and rep["unexpected"] == []
    assert all(float(fresh.state_dict()[k].abs().max()) == 0.0 for k in FT_KEYS)
    assert torch.equal(fresh.state_dict()[REG + "bbox.weight"].cpu(), stage1[REG + "bbox.weight"])
    # eval
    model.eval()
    model.compute_dtype = torch.float32
    sup, _ = synthetic_batch(2, 0, hw=HW, seed=8)
    inp = [{"image": s["image"]} for s in sup]
    out = _detections(model, inp)
    assert len(out) == 2 and all(len(o) > 0 for o in out)
    mbp = model.roi_heads.box_predictor
    with torch.no_grad():
        mbp.bbox_pred_ft.weight.zero_()
    out_ft = _detections(model, inp)
    assert _moved(out, out_ft), "bbox_pred_ft does not reach the decoded boxes"
    with torch.no_grad():
        mbp.weak_detector_head.regression_branch_bbox.weight.zero_()
        mbp.weak_detector_head.regression_branch_bbox.bias.zero_()
    out_w = _detections(model, inp)
    assert _moved(out_ft, out_w), "the weak deltas do not reach the decoded boxes"
