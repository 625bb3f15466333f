"""WEAK_DETECTOR.REGRESSION_BRANCH without a GPU: the conditions on tests/golden/regression_branch_golden.npz (asserted by its generator, and
again here on the committed file), the generator's recipe where the reference tree exists, the C ABI's three new entries, construction
(parameters, initialisation, the solver's group, what stays refused) and the checkpoint round trip."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GDIR = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GDIR)
G = np.load(os.path.join(GDIR, "regression_branch_golden.npz"))
TAGS = ("a", "b", "c", "d", "e")
FG, BG, MARGIN = 0.5, 0.1, 1e-5


def _iou(gt, boxes):
    """detectron2 pairwise_iou [gt, rows] in float32"""
    gt, boxes = torch.from_numpy(gt), torch.from_numpy(boxes)
    a1, a2 = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]), (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    wh = (torch.min(gt[:, None, 2:], boxes[None, :, 2:]) - torch.max(gt[:, None, :2], boxes[None, :, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    return torch.where(inter > 0, inter / (a1[:, None] + a2[None] - inter), torch.zeros(1))


# ---------------------------------------------------------------------------------------------------- the fixture
def test_fixture_holds_the_cases_in_fp32_and_int32():
    assert tuple(G["tags"]) == TAGS
    shapes = {"a": (0, 20, [70, 5]), "b": (0, 20, [37, 2]), "c": (0, 80, [33, 12]), "d": (1, 20, [40, 9]), "e": (1, 80, [37, 5])}
    for tag, (pcl, k, sizes) in shapes.items():
        assert int(G[f"{tag}/pcl"]) == pcl and int(G[f"{tag}/K"]) == k and G[f"{tag}/sizes"].tolist() == sizes
        r = sum(sizes)
        assert G[f"{tag}/mean_scores"].shape == (r, k + 1) and G[f"{tag}/gt_boxes"].shape == (r, 4) and G[f"{tag}/regression_bbox"].shape == (r, 4 * k)
    assert all(len(G[f"b/targets{i}"]) == 1 for i in range(2)) and len(G["a/targets0"]) > 1
    for tag in ("a", "d"):
        for kind in ("sl1_b0.5", "giou"):
            assert G[f"{tag}/{kind}/grad_regression_bbox"].shape == G[f"{tag}/regression_bbox"].shape
    for k in G.files:
        assert G[k].dtype in (np.float32, np.int32) or k == "tags", (k, G[k].dtype)
    assert os.path.getsize(os.path.join(GDIR, "regression_branch_golden.npz")) < (1 << 20)


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_decisions_keep_their_margin(tag):
    """every argmax the mean score feeds: top-1 minus top-2 of the column >= 1e-5 relative; every row: best minus second-best IoU, and best
    IoU against FG / BG_THRESHOLD, >= 1e-5 (rows that overlap no pseudo-GT are an exact 0.0 tie in any arithmetic; first wins)"""
    sizes, pcl = G[f"{tag}/sizes"].tolist(), int(G[f"{tag}/pcl"])
    idx = np.insert(np.cumsum(sizes), 0, 0)
    mean = torch.from_numpy(G[f"{tag}/mean_scores"])
    mean3 = torch.stack([torch.softmax(torch.from_numpy(G[f"{tag}/oicr{k}"]), -1) for k in range(3)], 0).mean(0)
    torch.testing.assert_close(mean, mean3, rtol=1e-6, atol=1e-8)
    for i, n in enumerate(sizes):
        rows = slice(idx[i], idx[i + 1])
        p = mean[rows].clone()
        for c in G[f"{tag}/targets{i}"].tolist():
            col = p[:, c]
            if n > 1:
                top = torch.sort(col, descending=True)[0]
                assert float(top[0] - top[1]) >= MARGIN * float(top[0]), (tag, i, c)
            if not pcl:
                p[int(torch.argmax(col))] = 0.0
        boxes, gtb = G[f"{tag}/boxes{i}"], G[f"{tag}/gt_boxes"][rows]
        pseudo = np.unique(gtb, axis=0)          # every pseudo-GT is one of the image's own boxes and matches itself
        q = _iou(pseudo, boxes)
        srt = torch.sort(q, dim=0, descending=True)[0]
        best = srt[0]
        if q.shape[0] > 1:
            gap = best - srt[1]
            assert not bool(((gap < MARGIN) & ~((best == 0) & (srt[1] == 0))).any()), (tag, i)
        for thr in (FG, BG):
            assert not bool(((best - thr).abs() < MARGIN).any()), (tag, i, thr)
        # the recorded decisions are those IoUs': label, weight 0 under BG_THRESHOLD, the matched box
        lab, w = G[f"{tag}/gt_classes"][rows], G[f"{tag}/cls_weights"][rows]
        k = int(G[f"{tag}/K"])
        assert np.array_equal(lab == k, (best < FG).numpy()) and np.array_equal(w == 0, (best < BG).numpy())
        assert np.array_equal(pseudo[q.argmax(0).numpy()][(best > 0).numpy()], gtb[(best > 0).numpy()])
    if tag == "b":
        assert bool((G["b/cls_weights"] == 0).any())


@pytest.mark.skipif(not os.path.isdir("/root/reference/modeling"), reason="the reference tree exists only in the authoring container")
def test_generator_reproduces_the_committed_fixture(tmp_path):
    out = str(tmp_path / "regen")
    r = subprocess.run([sys.executable, os.path.join(GDIR, "gen_regression_branch_golden.py"), out], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    new = np.load(os.path.join(out, "regression_branch_golden.npz"))
    assert sorted(new.files) == sorted(G.files)
    for k in G.files:
        a, b = new[k], G[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype.kind == "f":          # (test_golden_recipe_cpu.py: bit for bit but for torch's thread-pool re-association)
            np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=k)
        else:
            assert np.array_equal(a, b), k


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_the_three_new_entries():
    from unit_amd import _lib
    protos, names = _lib.parse_header(), _lib.parse_header_names()
    for name in ("unit_softmax_mean", "unit_oicr_targets_ex", "unit_pcl_targets_ex"):
        assert name in protos and names[name][-1] == "stream" and _lib.enqueues(name), name
    for plain in ("unit_oicr_targets", "unit_pcl_targets"):          # the _ex forms are the plain ones plus gt_boxes
        ex = names[plain + "_ex"]
        assert [n for n in ex if n != "gt_boxes"] == names[plain] and "gt_boxes" in ex
        assert len(protos[plain + "_ex"][1]) <= _lib.UnitCall.INTS + 4          # fits a recorded call (<= 32 integer words, 4 floats here)
    assert names["unit_softmax_mean"] == ["logits", "ld", "col0", "step", "n", "K", "valid", "out", "ldo", "R", "stream"]


# ---------------------------------------------------------------------------------------------------- construction
def _cfg(terms=("lingual",), **kw):
    import gen_ref_step as grs
    c = grs.case_cfg("s1")
    wd = c.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR
    for k, v in kw.items():
        setattr(wd, k, v)
    ft = c.MODEL.ROI_HEADS.FINETUNE_TERMS
    ft.CLASSIFIER, ft.BBOX, ft.MASK = list(terms), list(terms), list(terms)
    return c


@pytest.mark.parametrize("typ", ["OICR", "PCL"])
def test_switch_builds_the_references_parameters(typ):
    from unit_amd.modeling import build_model
    from unit_amd.modeling.rcnn import LOSS_NAMES
    on, off = build_model(_cfg(TYPE=typ, REGRESSION_BRANCH=True)), build_model(_cfg(TYPE=typ))
    pre = "roi_heads.box_predictor.weak_detector_head.regression_branch_"
    sd, k, d = on.state_dict(), 20, on.roi_heads.box_predictor.input_size
    new = {pre + "cls.weight": (k + 1, d), pre + "cls.bias": (k + 1,), pre + "bbox.weight": (4 * k, d), pre + "bbox.bias": (4 * k,)}
    assert {n: tuple(sd[n].shape) for n in new} == new
    assert sorted(set(sd) - set(off.state_dict())) == sorted(new)
    assert float(sd[pre + "cls.bias"].abs().max()) == 0 and float(sd[pre + "bbox.bias"].abs().max()) == 0
    assert 0.005 < float(sd[pre + "cls.weight"].std()) < 0.02 and 0.0005 < float(sd[pre + "bbox.weight"].std()) < 0.002          # std 0.01 / 0.001 (:96-97)
    bw = "roi_heads.box_predictor.bbox_pred_delta.weight"          # fast_rcnn.py:320-323
    assert float(sd[bw].abs().max()) == 0.0 and float(off.state_dict()[bw].abs().max()) > 0.0
    wh = on.roi_heads.box_predictor.weak_detector_head
    assert wh.group.members[-2:] == [wh.regression_branch_cls, wh.regression_branch_bbox] and len(wh.group.members) == 7          # one fused GEMM
    assert on.loss_names == LOSS_NAMES + ["loss_regression_cls", "loss_regression_bbox"] and off.loss_names == LOSS_NAMES
    assert build_model(_cfg(terms=(), TYPE=typ, REGRESSION_BRANCH=True)).roi_heads.terms["cls"] == []          # no transfer at all is fine too


def test_freeze_layers_reach_the_new_layers():
    from unit_amd.modeling import build_model
    c = _cfg(REGRESSION_BRANCH=True)
    c.MODEL.FREEZE_LAYERS.FAST_RCNN = ["weak_detector_head"]
    m = build_model(c)
    wh = m.roi_heads.box_predictor.weak_detector_head
    assert not any(p.requires_grad for p in wh.parameters())
    from unit_amd import config
    from unit_amd.modeling.fast_rcnn import WeakDetectorOutputsBase
    from unit_amd.structures import ShapeSpec
    c2 = config.get_cfg()
    c2.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR.REGRESSION_BRANCH = True
    c2.MODEL.FREEZE_LAYERS.FAST_RCNN = ["regression_branch_bbox"]
    w2 = WeakDetectorOutputsBase(c2, ShapeSpec(channels=128))
    assert not w2.regression_branch_bbox.weight.requires_grad and w2.regression_branch_cls.weight.requires_grad


def test_solver_puts_the_new_layers_in_the_weak_head_group():
    """solver.hyper_for: `regression_branch` modules take the refinement predictors' LR factor and weight decay, and nobody else's"""
    from unit_amd import solver
    from unit_amd.modeling import build_model
    c = _cfg(REGRESSION_BRANCH=True)
    s_ = c.SOLVER
    s_.REFINEMENT_LR_FACTOR, s_.MIL_LR_FACTOR, s_.DELTA_LR_FACTOR, s_.BIAS_LR_FACTOR = 3.0, 5.0, 7.0, 2.0
    names = [n for n, _ in build_model(c).named_parameters()]
    pre = "roi_heads.box_predictor.weak_detector_head."
    for layer in ("regression_branch_cls", "regression_branch_bbox"):
        for leaf in ("weight", "bias"):
            assert pre + f"{layer}.{leaf}" in names
            assert solver.hyper_for(c, pre + f"{layer}.{leaf}") == solver.hyper_for(c, pre + f"oicr_predictors.0.{leaf}")
    assert solver.hyper_for(c, pre + "regression_branch_cls.weight") == (3.0, s_.WEIGHT_DECAY)
    assert solver.hyper_for(c, pre + "regression_branch_bbox.bias") == (6.0, s_.WEIGHT_DECAY_BIAS)
    assert solver.hyper_for(c, "roi_heads.box_predictor.bbox_pred_delta.weight")[0] == 7.0


def test_what_stays_refused_says_what_remains():
    from unit_amd.modeling import build_model
    for typ in ("OICR", "PCL"):
        with pytest.raises(AssertionError, match="OICR_REGRESSION_BRANCH.*not supported"):
            build_model(_cfg(TYPE=typ, OICR_REGRESSION_BRANCH=True))
        for terms in (("lingual", "visual"), ("visual",)):
            with pytest.raises(ValueError, match="visual.*REGRESSION_BRANCH.*list of refinement streams"):
                build_model(_cfg(terms=terms, TYPE=typ, REGRESSION_BRANCH=True))
            with pytest.raises(AssertionError):          # ... and, like every other refusal at construction, an AssertionError
                build_model(_cfg(terms=terms, TYPE=typ, REGRESSION_BRANCH=True))
    import gen_ref_step as grs
    c = grs.case_cfg("s2")          # the fine-tune predictor
    c.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR.REGRESSION_BRANCH = True
    with pytest.raises(AssertionError, match="SupervisedDetectorOutputsFineTune with WEAK_DETECTOR.REGRESSION_BRANCH is not supported"):
        build_model(c)
    with pytest.raises(AssertionError, match="OICR_ITER > 0"):
        build_model(_cfg(REGRESSION_BRANCH=True, OICR_ITER=0))


def test_similarity_refuses_a_visual_term_set_after_construction():
    """the check sits where the matrix would be computed too: terms edited on a built model do not slip through"""
    from unit_amd.modeling import build_model
    from unit_amd.modeling.inference import similarity_dict
    m = build_model(_cfg(REGRESSION_BRANCH=True))
    m.roi_heads.terms = {"cls": ["lingual", "visual"], "bbox": ["lingual"]}
    m.roi_heads._role_cache = dict(dev=torch.device("cpu"), emb_novel=None, emb_base=None, base=None, novel=None)
    import unit_amd.ops as ops
    orig = ops.embedding_similarity
    ops.embedding_similarity = lambda *a: None
    try:
        with pytest.raises(ValueError, match="visual"):
            similarity_dict(m, None)
    finally:
        ops.embedding_similarity = orig


# ---------------------------------------------------------------------------------------------------- checkpoint
def test_checkpoint_round_trips_the_four_keys(tmp_path):
    from unit_amd import checkpoint
    from unit_amd.modeling import build_model
    torch.manual_seed(3)
    a = build_model(_cfg(REGRESSION_BRANCH=True))
    pre = "roi_heads.box_predictor.weak_detector_head.regression_branch_"
    keys = [pre + s for s in ("cls.weight", "cls.bias", "bbox.weight", "bbox.bias")]
    with torch.no_grad():
        for k in keys:
            a.state_dict()[k].copy_(torch.randn(a.state_dict()[k].shape))
    path = checkpoint.save_checkpoint(a, str(tmp_path / "m.pth"), iteration=7)
    saved = torch.load(path, weights_only=False)["model"]
    assert all(k in saved for k in keys)
    b = build_model(_cfg(REGRESSION_BRANCH=True))
    rep = checkpoint.load_checkpoint(b, path)
    assert not [k for k in rep["missing"] if "regression_branch" in k] and not rep["unexpected"] and rep["extras"]["iteration"] == 7
    for k in keys:
        assert torch.equal(a.state_dict()[k], b.state_dict()[k]), k
    # a reference checkpoint names them without this project's nesting changing anything: the suffix rule finds them
    ref_names = {k.replace("roi_heads.box_predictor.", "box_predictor."): v for k, v in saved.items() if "regression_branch" in k}
    c = build_model(_cfg(REGRESSION_BRANCH=True))
    rep = checkpoint.load_checkpoint(c, ref_names)
    assert all(torch.equal(a.state_dict()[k], c.state_dict()[k]) for k in keys) and not rep["unexpected"]
    # a model without the switch reports them as unexpected instead of loading them somewhere
    d = build_model(_cfg())
    assert sorted(checkpoint.load_checkpoint(d, path)["unexpected"]) == sorted(keys)
