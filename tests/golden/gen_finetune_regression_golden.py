"""Generates tests/golden/finetune_regression_golden.npz by RUNNING THE REFERENCE'S OWN SupervisedDetectorOutputsFineTune with
`regression_branch=True` (fast_rcnn.py:484-533; imported by file through d2_stubs.load_reference(), as gen_regression_branch_golden.py does,
whose helpers -- make_head, clustered_boxes, make_sup_proposals and the bound giou_loss -- are used here; the reference's text is not touched).

The arithmetic under test (fast_rcnn.py:504-528 with :360-364 and :370-374):
  scores = ((delta + transfer(delta)) + regression_branch_cls(x_weak)) + cls_score_ft(x)
  bbox   = ((base: delta | novel: sim . delta_base | else 0) + regression_branch_bbox(x_weak)) + bbox_pred_ft(x)
the weak head evaluated under no_grad (:490-494), the similarity applied in training as in eval, no -inf fill.

Cases (D = 32; every predictor weight random and NON-zero, the *_ft heads included -- with zero weights the ft add would be untested):
  F20  K = 20, VOC split-1 base / novel, sizes (31, 26)
  F80  K = 80, the COCO split of gen_unit_golden.py (the 20 VOC classes novel), sizes (33, 12); the similarity rows are sparse there (about
       nine entries in ten are exact zeros, as the thresholded visual term leaves them), dense in F20
  F1   K = 20, ONE RoI, whose gt class is novel
Per case `<tag>/...`:
  K, sizes, base, novel, x, xw, prop_boxes, prop_gt_boxes, prop_gt_classes, param/<name> (every parameter the forward reads);
  the six Linear outputs lin_delta_cls, lin_delta_bbox, lin_ft_cls, lin_ft_bbox, lin_weak_cls, lin_weak_bbox (the last two are the weak head's
  regression_branch_cls / regression_branch_bbox on xw): a kernel can be tested on them without any GEMM of the project's;
  sim_cls, sim_bbox [R, novel, base] (the 2-D similarity is row 0);
  scores_<m>, bbox_<m> for m in 3d / 2d / none: the forward in TRAINING mode. The forward in eval mode is asserted bit-equal to it here (the
  reference's FineTune.forward has no branch on self.training), so one copy serves both;
  loss_cls and <kind>/loss_box_reg for kind in sl1_b0 / sl1_b0.5 / giou on the 3d training forward; grad_cls_ft_out = d(total)/d(output of
  cls_score_ft) (the same under every kind: asserted) and <kind>/grad_bbox_ft_out = d(total)/d(output of bbox_pred_ft).

Conditions the generator asserts (tests/test_finetune_regression_cpu.py asserts those that can be read off the file again):
  * the gt classes of the proposals come from base AND novel: >= 3 foreground rows of each (F1: its one row is novel), >= a quarter background;
  * every loss is finite;
  * with the layers frozen that every *-ft.yaml freezes (weak_detector_head, cls_score_delta, bbox_pred_delta, embeddings) no gradient
    reaches a weak_detector_head or delta-head parameter, and the ft heads' parameters all get one;
  * with the ft heads zeroed, the TRAINING forward of the FineTune predictor is torch.equal to the EVAL forward of
    SupervisedDetectorOutputsBase(regression_branch=True) on the same state, for the 3-D and the 2-D similarity.
SEEDS: the first seeds (counting up from 501 / 511 / 521) at which the drawn gt classes satisfy the first condition (--search prints them).
fp32 and int32 only.
Run here:  python tests/golden/gen_finetune_regression_golden.py [out_dir]"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_regression_branch_golden as rb  # noqa: E402  (loads the reference once; giou_loss and _predict_boxes are bound there)

d2, REF, npy, D, BOX_WEIGHTS = rb.d2, rb.REF, rb.npy, rb.D, rb.BOX_WEIGHTS
KINDS = (("sl1_b0", "smooth_l1", 0.0), ("sl1_b0.5", "smooth_l1", 0.5), ("giou", "giou", 0.0))
FROZEN = ["weak_detector_head", "cls_score_delta", "bbox_pred_delta", "embeddings"]          # FREEZE_LAYERS.FAST_RCNN of every *-ft.yaml
COCO_NOVEL = [0, 1, 2, 3, 4, 5, 6, 8, 14, 15, 16, 17, 18, 19, 39, 56, 57, 58, 60, 62]      # gen_unit_golden.py: the VOC classes inside COCO
COCO_BASE = [i for i in range(80) if i not in COCO_NOVEL]
VOC_BASE, VOC_NOVEL = list(rb.gb.orc.VOC_BASE_SPLIT1), list(rb.gb.orc.VOC_NOVEL_SPLIT1)
# tag, K, sizes, base, novel, seed, fraction of similarity entries zeroed
CASES = [("F20", 20, (31, 26), VOC_BASE, VOC_NOVEL, 502, 0.0), ("F80", 80, (33, 12), COCO_BASE, COCO_NOVEL, 512, 0.9),
         ("F1", 20, (1,), VOC_BASE, VOC_NOVEL, 521, 0.0)]
READ = ("cls_score_delta", "bbox_pred_delta", "cls_score_ft", "bbox_pred_ft")


def make_predictor(cls_name, K, weak, emb, freeze):
    return getattr(REF["fast_rcnn"], cls_name)(
        d2.ShapeSpec(channels=D), box2box_transform=d2.Box2BoxTransform(BOX_WEIGHTS), num_classes=K, test_score_thresh=0.05, test_nms_thresh=0.5,
        test_topk_per_image=100, smooth_l1_beta=0.0, loss_weight={"loss_box_reg": 1.0}, weak_detector_head=weak, regression_branch=True,
        terms={"cls": ["lingual"], "bbox": ["lingual"], "seg": ["lingual"]}, freeze_layers=list(freeze), embedding_path=emb)


def similarity(g, R, n_novel, n_base, zeroed):
    s = torch.rand(R, n_novel, n_base, generator=g)
    if zeroed:
        keep = torch.rand(R, n_novel, n_base, generator=g) >= zeroed
        keep[..., 0] |= ~keep.any(-1)          # (no empty row)
        s = s * keep
    return s / s.sum(-1, keepdim=True)


def proposal_conditions(cls, K, base, novel, one_novel=False):
    """None, or why these gt classes are not a fixture"""
    fg_b, fg_n = sum(int(c) in base for c in cls.tolist()), sum(int(c) in novel for c in cls.tolist())
    if one_novel:
        return None if (len(cls) == 1 and fg_n == 1) else "the one row must carry a novel class"
    if fg_b < 3 or fg_n < 3:
        return f"{fg_b} base / {fg_n} novel foreground rows: at least 3 of each"
    if int((cls == K).sum()) * 4 < len(cls):
        return "less than a quarter of the rows is background"
    return None


def run_case(out, tag, K, sizes, base, novel, seed, zeroed):
    g = torch.Generator().manual_seed(seed)
    weak = rb.make_head("OICR", K, g)
    emb = os.path.join(tempfile.mkdtemp(), "emb.pth")
    torch.save({"embeddings": torch.randn(80, 300, generator=g)}, emb)          # get_similarity is not exercised here
    pred = make_predictor("SupervisedDetectorOutputsFineTune", K, weak, emb, FROZEN)
    amax = lambda p_: float(p_.detach().abs().max())
    assert amax(pred.bbox_pred_delta.weight) == 0.0          # fast_rcnn.py:322-323, FineTune under the switch as Base
    assert amax(pred.cls_score_ft.weight) == 0.0 and amax(pred.bbox_pred_ft.weight) == 0.0          # :480-482
    with torch.no_grad():
        for n_, p_ in pred.named_parameters():
            if not (n_.startswith("weak_detector_head") or n_.startswith("embeddings")):
                p_.copy_(torch.randn(p_.shape, generator=g) * (0.3 if p_.dim() > 1 else 0.1))
    assert all(float(getattr(pred, n_).weight.detach().abs().min()) > 0 for n_ in ("cls_score_ft", "bbox_pred_ft"))
    R = sum(sizes)
    x, xw = torch.randn(R, D, generator=g), torch.randn(R, D, generator=g)
    props, flat = rb.make_sup_proposals(g, list(sizes), K, sorted(base + novel))
    if tag == "F1":
        flat["gt_classes"][0] = novel[1]
        props[0].gt_classes = flat["gt_classes"].clone()
    why = proposal_conditions(flat["gt_classes"], K, base, novel, one_novel=tag == "F1")
    assert why is None, f"case {tag} seed {seed}: {why} -- reseed"
    nov_t, base_t = torch.tensor(novel), torch.tensor(base)
    out[f"{tag}/K"], out[f"{tag}/sizes"] = np.array(K, dtype=np.int32), np.array(sizes, dtype=np.int32)
    out[f"{tag}/base"], out[f"{tag}/novel"] = np.array(base, dtype=np.int32), np.array(novel, dtype=np.int32)
    out[f"{tag}/x"], out[f"{tag}/xw"] = npy(x), npy(xw)
    for k, v in flat.items():
        out[f"{tag}/prop_{k}"] = npy(v)
    for n_, v in pred.state_dict().items():
        if n_.split(".")[0] in READ or n_.startswith("weak_detector_head.regression_branch"):
            out[f"{tag}/param/{n_}"] = npy(v)
    sim3 = {"cls": similarity(g, R, len(novel), len(base), zeroed), "bbox": similarity(g, R, len(novel), len(base), zeroed)}
    sim2 = {k: v[0].clone() for k, v in sim3.items()}
    out[f"{tag}/sim_cls"], out[f"{tag}/sim_bbox"] = npy(sim3["cls"]), npy(sim3["bbox"])
    with torch.no_grad():
        for nm, mod, inp in (("delta_cls", pred.cls_score_delta, x), ("delta_bbox", pred.bbox_pred_delta, x), ("ft_cls", pred.cls_score_ft, x),
                             ("ft_bbox", pred.bbox_pred_ft, x), ("weak_cls", weak.regression_branch_cls, xw),
                             ("weak_bbox", weak.regression_branch_bbox, xw)):
            out[f"{tag}/lin_{nm}"] = npy(mod(inp))
    fwd = lambda p_, sim: p_(x, nov_t, base_t, supervised_branch_x_weak=xw, x_weak=None, similarity=sim)
    for nm, sim in (("3d", sim3), ("2d", sim2), ("none", None)):
        pred.train()
        with torch.no_grad():
            (st, bt), weak_ret = fwd(pred, sim)
            assert weak_ret is None and st.shape == (R, K + 1) and bt.shape == (R, 4 * K)
            assert bool(torch.isfinite(st).all()), "no novel column is filled with -inf"
            pred.eval()
            (se, be), _ = fwd(pred, sim)
        assert torch.equal(st, se) and torch.equal(bt, be), "FineTune.forward does not branch on self.training"
        out[f"{tag}/scores_{nm}"], out[f"{tag}/bbox_{nm}"] = npy(st), npy(bt)
    kept = {}

    def keep(name):
        def hook(mod, inp, o):
            o.retain_grad()
            kept[name] = o
        return hook
    hooks = [getattr(pred, n_).register_forward_hook(keep(n_)) for n_ in ("cls_score_ft", "bbox_pred_ft")]
    pred.train()
    first = None
    for kind, loss_type, beta in KINDS:
        pred.box_reg_loss_type, pred.smooth_l1_beta = loss_type, beta
        pred.zero_grad()
        (scores, bbox), _ = fwd(pred, sim3)
        losses = pred.losses([scores, bbox], props)
        assert set(losses) == {"loss_cls", "loss_box_reg"} and all(bool(torch.isfinite(v)) for v in losses.values()), (tag, kind, losses)
        sum(losses.values()).backward()
        for n_, p_ in pred.named_parameters():
            top = n_.split(".")[0]
            if top in ("weak_detector_head", "cls_score_delta", "bbox_pred_delta"):
                assert p_.grad is None, f"{n_} received a gradient"
            elif top in ("cls_score_ft", "bbox_pred_ft"):
                assert p_.grad is not None and float(p_.grad.abs().max()) > 0, n_
        gc_, gb_ = kept["cls_score_ft"].grad, kept["bbox_pred_ft"].grad
        if first is None:
            first = (losses["loss_cls"].detach().clone(), gc_.clone())
            out[f"{tag}/loss_cls"], out[f"{tag}/grad_cls_ft_out"] = npy(losses["loss_cls"]), npy(gc_)
        assert torch.equal(losses["loss_cls"].detach(), first[0]) and torch.equal(gc_, first[1])
        out[f"{tag}/{kind}/loss_box_reg"], out[f"{tag}/{kind}/grad_bbox_ft_out"] = npy(losses["loss_box_reg"]), npy(gb_)
        assert float(gb_.abs().max()) > 0
        print(tag, kind, {k: round(v.item(), 6) for k, v in losses.items()}, flush=True)
    for h in hooks:
        h.remove()
    pred.box_reg_loss_type, pred.smooth_l1_beta = "smooth_l1", 0.0
    # the ft heads zeroed: the Base predictor's eval forward with the switch, which regression_branch_golden.npz pins
    state = {k: v.clone() for k, v in pred.state_dict().items()}
    with torch.no_grad():
        for n_ in ("cls_score_ft", "bbox_pred_ft"):
            getattr(pred, n_).weight.zero_(), getattr(pred, n_).bias.zero_()
    base_pred = make_predictor("SupervisedDetectorOutputsBase", K, weak, emb, [])
    base_pred.load_state_dict({k: v for k, v in state.items() if not k.split(".")[0].endswith("_ft")})
    pred.train(), base_pred.eval()
    with torch.no_grad():
        for sim in (sim3, sim2):
            (s0, b0), _ = fwd(pred, sim)
            (s1, b1), _ = fwd(base_pred, sim)
            assert torch.equal(s0, s1) and torch.equal(b0, b1), f"{tag}: FineTune with zeroed ft heads is not Base's eval forward"


def main(out_dir=HERE):
    torch.set_num_threads(1)
    out = {}
    for case in CASES:
        run_case(out, *case)
    out["tags"] = np.array([c[0] for c in CASES])
    assert all(v.dtype in (np.float32, np.int32) or v.dtype.kind == "U" for v in out.values())
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "finetune_regression_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


def search():
    """prints, per case, the first seed from the case's base at which the drawn gt classes satisfy the fixture conditions"""
    torch.set_num_threads(1)
    for tag, K, sizes, base, novel, seed, zeroed in CASES:
        for s in range(seed - seed % 10 + 1, seed - seed % 10 + 60):
            try:
                run_case({}, tag, K, sizes, base, novel, s, zeroed)
            except AssertionError as e:
                if "reseed" not in str(e):
                    raise
                print(tag, s, e)
                continue
            print(tag, "seed", s)
            break


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--search":
        search()
        sys.exit(0)
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
