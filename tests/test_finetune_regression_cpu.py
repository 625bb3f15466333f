"""The fine-tune predictor with WEAK_DETECTOR.REGRESSION_BRANCH without a GPU: the conditions on tests/golden/finetune_regression_golden.npz
(asserted by its generator, and again here on the committed file where the file alone shows them), the generator's recipe where the reference
tree exists, what builds and what stays refused, the C ABI's new entry, which entry `ops.transfer_predictions` issues, and the two checkpoint
cases (stage 2 -> stage 2, stage 1 -> stage 2)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GDIR = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GDIR)
PATH = os.path.join(GDIR, "finetune_regression_golden.npz")
G = np.load(PATH)
TAGS = ("F20", "F80", "F1")
KINDS = ("sl1_b0", "sl1_b0.5", "giou")
FT_KEYS = ["roi_heads.box_predictor." + n for n in ("cls_score_ft.weight", "cls_score_ft.bias", "bbox_pred_ft.weight", "bbox_pred_ft.bias")]
REG = "roi_heads.box_predictor.weak_detector_head.regression_branch_"


def T(k):
    return torch.from_numpy(G[k])


# ---------------------------------------------------------------------------------------------------- the fixture
def test_fixture_holds_the_three_cases_in_fp32_and_int32():
    from unit_amd import config
    assert tuple(G["tags"]) == TAGS
    shapes = {"F20": (20, [31, 26], 15, 5), "F80": (80, [33, 12], 60, 20), "F1": (20, [1], 15, 5)}
    for tag, (k, sizes, nb, nn_) in shapes.items():
        r = sum(sizes)
        assert int(G[f"{tag}/K"]) == k and G[f"{tag}/sizes"].tolist() == sizes
        assert len(G[f"{tag}/base"]) == nb and len(G[f"{tag}/novel"]) == nn_ and not set(G[f"{tag}/base"]) & set(G[f"{tag}/novel"])
        assert G[f"{tag}/x"].shape == (r, 32) and G[f"{tag}/xw"].shape == (r, 32)
        assert G[f"{tag}/sim_cls"].shape == (r, nn_, nb) == G[f"{tag}/sim_bbox"].shape
        for nm in ("3d", "2d", "none"):
            assert G[f"{tag}/scores_{nm}"].shape == (r, k + 1) and G[f"{tag}/bbox_{nm}"].shape == (r, 4 * k)
        for nm in ("delta", "ft", "weak"):
            assert G[f"{tag}/lin_{nm}_cls"].shape == (r, k + 1) and G[f"{tag}/lin_{nm}_bbox"].shape == (r, 4 * k)
        for kind in KINDS:
            assert G[f"{tag}/{kind}/grad_bbox_ft_out"].shape == (r, 4 * k)
    c = config.voc_rcnn_c4_split1_ft(50)
    assert G["F20/base"].tolist() == list(c.DATASETS.FEWSHOT.BASE_CLASSES_ID) and G["F20/novel"].tolist() == list(c.DATASETS.FEWSHOT.NOVEL_CLASSES_ID)
    assert G["F80/novel"].tolist() == config.COCO_SPLIT1_NOVEL and G["F80/base"].tolist() == config.COCO_SPLIT1_BASE
    for k in G.files:
        assert G[k].dtype in (np.float32, np.int32) or k == "tags", (k, G[k].dtype)
    assert os.path.getsize(PATH) < (1 << 20)


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_conditions(tag):
    """gt classes from base AND novel, a quarter background, finite losses, NON-zero ft heads (values and gradients), no -inf column"""
    k, cls = int(G[f"{tag}/K"]), G[f"{tag}/prop_gt_classes"]
    base, novel = set(G[f"{tag}/base"].tolist()), set(G[f"{tag}/novel"].tolist())
    fg_b, fg_n = sum(int(c) in base for c in cls), sum(int(c) in novel for c in cls)
    if tag == "F1":
        assert len(cls) == 1 and fg_n == 1
    else:
        assert fg_b >= 3 and fg_n >= 3 and int((cls == k).sum()) * 4 >= len(cls), (fg_b, fg_n, int((cls == k).sum()), len(cls))
    assert np.isfinite(G[f"{tag}/loss_cls"]) and all(np.isfinite(G[f"{tag}/{kind}/loss_box_reg"]) for kind in KINDS)
    for n in ("cls_score_ft", "bbox_pred_ft", "cls_score_delta", "bbox_pred_delta", "weak_detector_head.regression_branch_cls",
              "weak_detector_head.regression_branch_bbox"):
        assert float(np.abs(G[f"{tag}/param/{n}.weight"]).min()) > 0, n
    assert float(np.abs(G[f"{tag}/lin_ft_cls"]).max()) > 0.1 and float(np.abs(G[f"{tag}/lin_ft_bbox"]).max()) > 0.1
    for nm in ("3d", "2d", "none"):
        assert np.isfinite(G[f"{tag}/scores_{nm}"]).all() and np.isfinite(G[f"{tag}/bbox_{nm}"]).all()
    fg = (cls >= 0) & (cls < k)
    for kind in KINDS:          # the box gradient sits in the foreground rows' gt-class columns and nowhere else
        g = G[f"{tag}/{kind}/grad_bbox_ft_out"]
        assert float(np.abs(g[~fg]).max(initial=0.0)) == 0.0 and float(np.abs(g[fg]).max()) > 0
    torch.testing.assert_close(T(f"{tag}/sim_cls").sum(-1), torch.ones(T(f"{tag}/sim_cls").shape[:2]), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_is_the_references_order_of_additions(tag):
    """the recorded outputs are (o + weak) + ft of the recorded Linear outputs, bit for bit, wherever o is one value (no similarity: every
    column; with one: background, base classes); (o + ft) + weak -- the order of unit_transfer_predictions followed by add_weak_deltas -- is
    NOT, so a test that asks for equality there tells the two apart"""
    k = int(G[f"{tag}/K"])
    d_c, d_b, f_c, f_b, w_c, w_b = (T(f"{tag}/lin_{a}_{b}") for a in ("delta", "ft", "weak") for b in ("cls", "bbox"))
    assert torch.equal((d_c + w_c) + f_c, T(f"{tag}/scores_none")) and torch.equal((d_b + w_b) + f_b, T(f"{tag}/bbox_none"))
    base = T(f"{tag}/base").long()
    cols = torch.cat([base, torch.tensor([k])])
    bcols = (4 * base[:, None] + torch.arange(4)).flatten()
    for nm in ("3d", "2d"):
        assert torch.equal(((d_c + w_c) + f_c)[:, cols], T(f"{tag}/scores_{nm}")[:, cols])
        assert torch.equal(((d_b + w_b) + f_b)[:, bcols], T(f"{tag}/bbox_{nm}")[:, bcols])
    other = (d_b + f_b) + w_b
    frac = float((other != T(f"{tag}/bbox_none")).float().mean())
    print(f"{tag}: (o + ft) + weak differs from the reference in {100 * frac:.1f} % of the box deltas")
    assert frac > 0.05
    # novel columns carry the transfer: sim . delta_base, then the same two additions
    novel = T(f"{tag}/novel").long()
    tr = torch.bmm(T(f"{tag}/sim_cls"), d_c[:, base].unsqueeze(2)).squeeze(2)
    torch.testing.assert_close((((d_c[:, novel] + tr) + w_c[:, novel]) + f_c[:, novel]), T(f"{tag}/scores_3d")[:, novel], rtol=1e-5, atol=1e-5)
    trb = torch.bmm(T(f"{tag}/sim_bbox"), d_b.view(-1, k, 4)[:, base])
    want = (trb + w_b.view(-1, k, 4)[:, novel]) + f_b.view(-1, k, 4)[:, novel]
    torch.testing.assert_close(want, T(f"{tag}/bbox_3d").view(-1, k, 4)[:, novel], rtol=1e-5, atol=1e-5)
    assert float((T(f"{tag}/bbox_3d").view(-1, k, 4)[:, novel] - T(f"{tag}/bbox_none").view(-1, k, 4)[:, novel]).abs().max()) > 0.1


@pytest.mark.skipif(not os.path.isdir("/root/reference/modeling"), reason="the reference tree exists only in the authoring container")
def test_generator_reproduces_the_committed_fixture(tmp_path):
    """runs the reference again: the generator's own assertions (no gradient into the frozen heads, zeroed ft heads == Base's eval forward,
    training forward == eval forward) hold, and the file it writes is the committed one"""
    out = str(tmp_path / "regen")
    r = subprocess.run([sys.executable, os.path.join(GDIR, "gen_finetune_regression_golden.py"), out], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    new = np.load(os.path.join(out, "finetune_regression_golden.npz"))
    assert sorted(new.files) == sorted(G.files)
    for k in G.files:
        a, b = new[k], G[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype.kind == "f":          # (test_golden_recipe_cpu.py: bit for bit but for torch's thread-pool re-association)
            np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=k)
        else:
            assert np.array_equal(a, b), k


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_the_ex_entry():
    from unit_amd import _lib
    protos, names = _lib.parse_header(), _lib.parse_header_names()
    ex, plain = names["unit_transfer_predictions_ex"], names["unit_transfer_predictions"]
    assert [n for n in ex if n != "wbcol0"] == plain and ex.index("wbcol0") == plain.index("n_oicr") + 1
    assert ex[-1] == "stream" and _lib.enqueues("unit_transfer_predictions_ex")
    assert len(protos["unit_transfer_predictions_ex"][1]) <= _lib.UnitCall.INTS          # fits a recorded call (no float word)
    assert "unit_transfer_predictions_ex" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_ops_issue_the_ex_entry_only_when_asked(monkeypatch):
    """calls without wbcol0 keep issuing unit_transfer_predictions with the arguments they passed before: every configuration that runs
    today records the call list it records today"""
    from unit_amd import ops
    calls = []

    class Lib:
        def __getattr__(self, name):
            return lambda *a: calls.append((name, a)) or 0
    monkeypatch.setattr(ops, "lib", lambda: Lib())
    monkeypatch.setattr(ops, "_p", lambda t: None if t is None else id(t))
    monkeypatch.setattr(ops, "_s", lambda: 0)
    lin, weak, ft, idx = torch.zeros(3, 112), torch.zeros(3, 208), torch.zeros(3, 104), torch.zeros(2, dtype=torch.int32)
    args = (lin, 0, 21, 20, weak, 5, 3, None, None, idx, idx, idx, idx)
    ops.transfer_predictions(*args, ft=ft, fccol0=0, fbcol0=21)
    ops.transfer_predictions(*args, ft=ft, fccol0=0, fbcol0=21, wbcol0=-1)
    ops.transfer_predictions(*args, ft=ft, fccol0=0, fbcol0=21, wbcol0=126)
    assert [c[0] for c in calls] == ["unit_transfer_predictions", "unit_transfer_predictions_ex", "unit_transfer_predictions_ex"]
    plain, ex = calls[0][1], calls[2][1]
    assert len(plain) == 27 and len(ex) == 28 and ex[9] == 126 and calls[1][1][9] == -1
    strip = lambda a: [v for i, v in enumerate(a) if i not in (21, 23)]          # (the two fresh output buffers)
    assert strip(ex[:9] + ex[10:]) == strip(plain)


# ---------------------------------------------------------------------------------------------------- construction
def _cfg(name="s2", terms=("lingual",), on=True, **kw):
    import gen_ref_step as grs
    c = grs.case_cfg(name)
    wd = c.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR
    wd.REGRESSION_BRANCH = on
    for k, v in kw.items():
        setattr(wd, k, v)
    if terms is not None:
        ft = c.MODEL.ROI_HEADS.FINETUNE_TERMS
        ft.CLASSIFIER, ft.BBOX, ft.MASK = list(terms), list(terms), list(terms)
    return c


@pytest.mark.parametrize("name", ["s2", "mask_ft"])
def test_finetune_config_with_the_switch_builds(name):
    from unit_amd.modeling import build_model
    from unit_amd.modeling.fast_rcnn import SupervisedDetectorOutputsFineTune
    on, off = build_model(_cfg(name)), build_model(_cfg(name, on=False))
    bp = on.roi_heads.box_predictor
    assert type(bp) is SupervisedDetectorOutputsFineTune and bp.regression_branch and bp.weak_bbox_col == bp.weak_detector_head.col_reg_bbox
    assert off.roi_heads.box_predictor.weak_bbox_col is None
    sd = on.state_dict()
    assert all(k in sd for k in FT_KEYS) and all((REG + s) in sd for s in ("cls.weight", "cls.bias", "bbox.weight", "bbox.bias"))
    assert float(sd["roi_heads.box_predictor.bbox_pred_delta.weight"].abs().max()) == 0.0          # fast_rcnn.py:322-323, as Base
    assert float(off.state_dict()["roi_heads.box_predictor.bbox_pred_delta.weight"].abs().max()) > 0.0
    assert all(float(sd[k].abs().max()) == 0.0 for k in FT_KEYS)          # :480-482
    # the frozen-predictor condition of the fine-tune step holds with the four regression_branch_* parameters present
    trainable = [n for n, p in bp.named_parameters() if p.requires_grad]
    assert sorted(trainable) == ["bbox_pred_ft.bias", "bbox_pred_ft.weight", "cls_score_ft.bias", "cls_score_ft.weight"]
    assert bp.weak_detector_head.score_cols == (bp.weak_detector_head.col_reg_cls, 1)


def test_base_predictor_keeps_its_two_launch_form():
    import gen_ref_step as grs
    from unit_amd.modeling import build_model
    c = grs.case_cfg("s1")
    c.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR.REGRESSION_BRANCH = True
    ft = c.MODEL.ROI_HEADS.FINETUNE_TERMS
    ft.CLASSIFIER, ft.BBOX, ft.MASK = ["lingual"], ["lingual"], ["lingual"]
    bp = build_model(c).roi_heads.box_predictor
    assert bp.regression_branch and not bp.finetune and bp.weak_bbox_col is None


def test_what_stays_refused():
    from unit_amd.modeling import build_model
    from unit_amd.modeling.inference import UnsupportedConfig
    for name in ("s2", "mask_ft"):
        with pytest.raises(UnsupportedConfig, match="FINETUNE_TERMS") as e:          # the shipped default lists hold "visual"
            build_model(_cfg(name, terms=None))
        msg = str(e.value)          # names the three lists to set, then says why with the present "visual" message
        assert all(w in msg for w in ("FINETUNE_TERMS.CLASSIFIER", "FINETUNE_TERMS.BBOX", "FINETUNE_TERMS.MASK", "lingual"))
        assert "visual" in msg and "list of refinement streams" in msg
        for terms in (("lingual", "VisualK-2"), ("visual",)):
            with pytest.raises(UnsupportedConfig, match="REGRESSION_BRANCH"):
                build_model(_cfg(name, terms=terms))
        with pytest.raises(AssertionError, match="OICR_REGRESSION_BRANCH.*not supported"):
            build_model(_cfg(name, OICR_REGRESSION_BRANCH=True))
    for path in ("unit_amd/modeling/fast_rcnn.py", "README.md", "DESIGN.md"):          # the old refusal is gone from code and docs
        assert "the fine-tune stage on top of the weak regression branch is not built" not in open(os.path.join(ROOT, path)).read()
    import gen_ref_step as grs
    c1 = grs.case_cfg("s1")          # stage 1 keeps the present message, without the fine-tune opening
    c1.MODEL.ROI_HEADS.FAST_RCNN.WEAK_DETECTOR.REGRESSION_BRANCH = True
    with pytest.raises(UnsupportedConfig, match="^a \"visual\" term"):
        build_model(c1)
    m = build_model(_cfg("s2"))
    bp = m.roi_heads.box_predictor
    with pytest.raises(NotImplementedError, match="train_only_weak"):
        bp._forward_values(None, [], [])
    with pytest.raises(NotImplementedError, match="TTA"):
        bp.inference([None, None], [], tta=True)


# ---------------------------------------------------------------------------------------------------- checkpoint
def test_checkpoint_stage2_round_trip_and_stage1_into_stage2(tmp_path):
    from unit_amd import checkpoint
    from unit_amd.modeling import build_model
    torch.manual_seed(5)
    a = build_model(_cfg("s2"))
    reg_keys = [REG + s for s in ("cls.weight", "cls.bias", "bbox.weight", "bbox.bias")]
    with torch.no_grad():
        for k in reg_keys + FT_KEYS:
            a.state_dict()[k].copy_(torch.randn(a.state_dict()[k].shape))
    path = checkpoint.save_checkpoint(a, str(tmp_path / "ft.pth"), iteration=3)
    b = build_model(_cfg("s2"))
    rep = checkpoint.load_checkpoint(b, path)
    assert rep["missing"] == [] and rep["unexpected"] == []
    assert all(torch.equal(a.state_dict()[k], b.state_dict()[k]) for k in reg_keys + FT_KEYS)
    # stage 1 of a switch-on model: SupervisedDetectorOutputsBase, no *_ft keys
    s1 = build_model(_cfg("s1"))
    stage1 = {k: v.detach().clone() for k, v in s1.state_dict().items()}
    assert not any("_ft." in k for k in stage1) and all(k in stage1 for k in reg_keys)
    c = build_model(_cfg("s2"))
    rep = checkpoint.load_checkpoint(c, stage1)
    assert sorted(rep["missing"]) == sorted(FT_KEYS) and rep["unexpected"] == []
    assert all(float(c.state_dict()[k].abs().max()) == 0.0 for k in FT_KEYS)
    assert all(torch.equal(stage1[k], c.state_dict()[k]) for k in reg_keys)
