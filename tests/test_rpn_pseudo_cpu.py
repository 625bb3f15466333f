"""WeaklySupervisedRCNNRPN (meta_arch/rcnn.py:544-654) without a GPU: registry, signature, config defaults, refusals, state-dict keys,
and the fixture tests/golden/rpn_pseudo_golden.npz (the reference's own forward, tests/golden/gen_rpn_pseudo_golden.py) against a numpy
restatement of the selection (:594-599) and of the loss combination (:601-609, :622-624)."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

GDIR = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GDIR)
import gen_rpn_pseudo_golden as P  # noqa: E402

FX = np.load(os.path.join(GDIR, "rpn_pseudo_golden.npz"))
HAS_REF = os.path.isdir("/root/reference/modeling")


def _cfg(**kw):
    from unit_amd import config
    c = config.voc_rcnn_c4_split1(50)
    c.MODEL.DEVICE = "cpu"
    c.MODEL.META_ARCHITECTURE = "WeaklySupervisedRCNNRPN"
    for k, v in kw.items():
        node = c
        parts = k.split(".")
        for a in parts[:-1]:
            node = node[a]
        node[parts[-1]] = v
    return c


# ---------------------------------------------------------------------------------------------------- surface
def test_registered_with_the_base_class_signature():
    from unit_amd.modeling import build_model
    from unit_amd.modeling.rcnn import WeaklySupervisedRCNNNoMeta, WeaklySupervisedRCNNRPN
    from unit_amd.structures import META_ARCH_REGISTRY
    assert META_ARCH_REGISTRY.get("WeaklySupervisedRCNNRPN") is WeaklySupervisedRCNNRPN
    assert issubclass(WeaklySupervisedRCNNRPN, WeaklySupervisedRCNNNoMeta)
    sig = inspect.signature(WeaklySupervisedRCNNRPN.forward)
    assert str(sig) == "(self, batched_inputs, weak_batched_inputs=None, return_similarity=False, train_only_weak=False)"
    assert WeaklySupervisedRCNNRPN.inference is WeaklySupervisedRCNNNoMeta.inference          # the reference inherits it unchanged
    m = build_model(_cfg())
    assert type(m) is WeaklySupervisedRCNNRPN
    assert (m.weak_rpn_score_threshold, m.train_proposal_regressor, m.weak_proposal_divisor) == (0.99, True, 1.0)


def test_the_four_defaults_are_the_reference_values():
    from unit_amd import config
    c = config.get_cfg()
    assert c.MODEL.PROPOSAL_GENERATOR.WEAK_RPN_SCORE_TRESHOLD == 0.99
    assert c.MODEL.ROI_HEADS.TRAIN_USING_WEAK is False
    assert c.MODEL.ROI_HEADS.TRAIN_PROPOSAL_REGRESSOR is True
    assert c.MODEL.ROI_HEADS.WEAK_PROPOSAL_DIVISOR == 1.0 and isinstance(c.MODEL.ROI_HEADS.WEAK_PROPOSAL_DIVISOR, float)


@pytest.mark.skipif(not os.path.isdir("/root/reference/configs"), reason="the reference tree exists only in the authoring container")
def test_the_four_defaults_equal_default_config_py_as_text():
    from unit_amd import config
    txt = open("/root/reference/configs/default_config.py").read()
    c = config.get_cfg()
    for key in ("MODEL.PROPOSAL_GENERATOR.WEAK_RPN_SCORE_TRESHOLD", "MODEL.ROI_HEADS.TRAIN_USING_WEAK", "MODEL.ROI_HEADS.TRAIN_PROPOSAL_REGRESSOR",
                "MODEL.ROI_HEADS.WEAK_PROPOSAL_DIVISOR"):
        m = re.search(r"^\s*_C\." + re.escape(key) + r"\s*=\s*(\S+)\s*$", txt, flags=re.M)
        assert m, key
        node = c
        for a in key.split("."):
            node = node[a]
        ref = {"True": True, "False": False}.get(m.group(1), None)
        ref = float(m.group(1)) if ref is None else ref
        assert node == ref and type(node) is type(ref), (key, node, m.group(1))


def test_loss_names_gain_two_slots_for_this_class_only():
    from unit_amd.modeling import build_model
    from unit_amd.modeling.rcnn import LOSS_NAMES, WEAK_RPN_LOSSES
    c = _cfg()
    rpn = build_model(c)
    assert rpn.loss_names == LOSS_NAMES + ["weak_loss_rpn_cls", "weak_loss_rpn_loc"] == LOSS_NAMES + WEAK_RPN_LOSSES
    c.MODEL.META_ARCHITECTURE = "WeaklySupervisedRCNNNoMeta"
    base = build_model(c)
    assert base.loss_names == LOSS_NAMES
    assert sorted(rpn.state_dict()) == sorted(base.state_dict())
    assert [n for n, _ in rpn.named_parameters()] == [n for n, _ in base.named_parameters()]


def test_refusals_name_their_reason():
    from unit_amd.modeling import build_model
    from unit_amd.modeling.inference import UnsupportedConfig
    with pytest.raises(UnsupportedConfig, match="TRAIN_USING_WEAK.*return_proposals"):
        build_model(_cfg(**{"MODEL.ROI_HEADS.TRAIN_USING_WEAK": True}))
    with pytest.raises(UnsupportedConfig, match="must name an RPN.*PrecomputedProposals"):
        build_model(_cfg(**{"MODEL.PROPOSAL_GENERATOR.NAME": "PrecomputedProposals"}))
    with pytest.raises(UnsupportedConfig, match="DETECTIONS_PER_IMAGE > 256"):
        build_model(_cfg(**{"TEST.DETECTIONS_PER_IMAGE": 300}))
    # the base class still meets an unknown proposal generator with the registry's KeyError
    c = _cfg(**{"MODEL.PROPOSAL_GENERATOR.NAME": "PrecomputedProposals"})
    c.MODEL.META_ARCHITECTURE = "WeaklySupervisedRCNNNoMeta"
    with pytest.raises(KeyError):
        build_model(c)


def test_graph_and_replay_refuse_the_class_at_construction():
    from unit_amd import engine
    from unit_amd.modeling import build_model
    m = build_model(_cfg())
    for cls in (engine.GraphedStep, engine.ReplayedStep):
        with pytest.raises(NotImplementedError, match="runs eagerly only.*Missing: the weak half"):
            cls(m, optimizer=None)


def test_header_declares_the_two_new_entries():
    from unit_amd import _lib
    protos, names = _lib.parse_header(), _lib.parse_header_names()
    assert names["unit_pseudo_gt"] == ["boxes", "scores", "cls", "count", "multihot", "B", "T", "K", "threshold", "gt_boxes", "gt_count", "kept_idx", "stream"]
    assert names["unit_gate_anchor_labels"] == ["labels", "gt_count", "B", "Ncap", "stream"]
    for n in ("unit_pseudo_gt", "unit_gate_anchor_labels"):
        assert _lib.enqueues(n) and len(protos[n][1]) <= _lib.UnitCall.INTS
    hdr = open(_lib.HEADER).read()
    assert "rcnn.py:594-599" in hdr[hdr.index("unit_pseudo_gt") - 600: hdr.index("int unit_pseudo_gt")]


# ---------------------------------------------------------------------------------------------------- the fixture
def test_fixture_conditions_hold():
    """one weak image keeps >= 2 pseudo GT, the other none; a detection dropped by label, one by score; both weak losses non-zero ("on"),
    the loc loss exactly 0 ("off"); every label-matching score keeps the bf16 margin from the threshold"""
    P.check_conditions(FX)
    thr = float(FX["threshold"])
    for i in range(2):
        sc, m = FX[f"on/weak/det_scores{i}"], np.isin(FX[f"on/weak/det_classes{i}"], FX[f"on/weak/labels{i}"])
        assert (np.abs(sc[m] - thr) > P.BF16_MARGIN * thr).all()
    assert P.BF16_MARGIN >= 4 * 2.0 ** -8          # a bf16 rounding moves a value by at most 2^-9 relative; a few of them in a row stay inside


@pytest.mark.parametrize("tag", P.CASES)
def test_selection_restated_reproduces_the_reference_pseudo_gt(tag):
    thr = float(FX["threshold"])
    for i in range(2):
        sc, cl, lab = FX[f"{tag}/weak/det_scores{i}"], FX[f"{tag}/weak/det_classes{i}"], FX[f"{tag}/weak/labels{i}"]
        kept = P.select(sc, cl, lab, thr)
        assert np.array_equal(kept, FX[f"{tag}/weak/kept{i}"]), (tag, i)
        assert np.array_equal(FX[f"{tag}/weak/det_boxes{i}"][kept], FX[f"{tag}/weak/pseudo_boxes{i}"])
        assert (f"{tag}/weak/anchor_labels{i}" in FX.files) == (len(kept) > 0)          # the proposal generator runs only with pseudo GT (:600)


@pytest.mark.parametrize("tag", P.CASES)
def test_loss_combination_restated_reproduces_the_two_scalars(tag):
    """:601-609, :622-624: per image loss x threshold x divisor (loc: x 0.0 with the regressor off), 0 for an image without pseudo GT,
    mean over the weak images -- from the fixture's per-image losses (already / (BATCH_SIZE_PER_IMAGE x 1), x loss_weight 1.0)"""
    thr, div = float(FX["threshold"]), float(FX["divisor"])
    cls, loc = [], []
    for i in range(2):
        key = f"{tag}/weak/image_losses{i}"
        if key in FX.files:
            cls.append(FX[key][0] * thr * div)
            loc.append(FX[key][1] * thr * div if tag == "on" else FX[key][1] * 0.0)
        else:
            cls.append(0.0)
            loc.append(0.0)
    names = [str(n) for n in FX[f"{tag}/loss_names"]]
    got = dict(zip(names, FX[f"{tag}/losses"]))
    assert abs(np.mean(cls) - got["weak_loss_rpn_cls"]) <= 1e-6 * abs(got["weak_loss_rpn_cls"])
    assert abs(np.mean(loc) - got["weak_loss_rpn_loc"]) <= 1e-6 * abs(got["weak_loss_rpn_loc"])
    assert set(names) == {"loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc", "weak_loss_rpn_cls", "weak_loss_rpn_loc"}      # :644: no weak ROI-head losses


def test_fixture_weak_anchor_labels_are_a_sample_against_the_pseudo_gt():
    for i in range(2):
        key = f"on/weak/anchor_labels{i}"
        if key in FX.files:
            lab = FX[key]
            assert lab.dtype == np.int8 and set(np.unique(lab)) <= {-1, 0, 1}
            assert 1 <= (lab == 1).sum() <= 128 and (lab >= 0).sum() == 256
    assert np.array_equal(FX["on/weak/anchor_labels0"] if "on/weak/anchor_labels0" in FX.files else FX["on/weak/anchor_labels1"],
                          FX["off/weak/anchor_labels0"] if "off/weak/anchor_labels0" in FX.files else FX["off/weak/anchor_labels1"])


def test_fixture_records_the_rpn_head_gradients_and_no_weak_head_gradient():
    for tag in P.CASES:
        for n in ("conv.weight", "conv.bias", "objectness_logits.weight", "objectness_logits.bias", "anchor_deltas.weight", "anchor_deltas.bias"):
            assert float(FX[f"{tag}/gradnorm/proposal_generator.rpn_head.{n}"]) > 0
        assert f"{tag}/gradnorm/backbone.res4.5.conv1.weight" in FX.files
        assert not any("weak_box_head" in k or "weak_detector_head" in k for k in FX.files if k.startswith(f"{tag}/gradnorm/"))
    # the regressor switch only removes the weak loc term: the objectness gradient is the same, the deltas' differs
    a, b = "on/gradhead/proposal_generator.rpn_head.", "off/gradhead/proposal_generator.rpn_head."
    assert np.array_equal(FX[a + "objectness_logits.bias"], FX[b + "objectness_logits.bias"])
    assert not np.array_equal(FX[a + "anchor_deltas.bias"], FX[b + "anchor_deltas.bias"])


@pytest.mark.skipif(not HAS_REF, reason="the reference tree exists only in the authoring container")
def test_generator_reproduces_the_committed_fixture(tmp_path):
    out = str(tmp_path / "regen.npz")
    r = subprocess.run([sys.executable, os.path.join(GDIR, "gen_rpn_pseudo_golden.py"), out], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    new = np.load(out)
    assert sorted(new.files) == sorted(FX.files)
    for k in FX.files:
        a, b = new[k], FX[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype.kind == "f":          # (test_golden_recipe_cpu.py: bit for bit but for torch's thread-pool re-association)
            np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=k)
        else:
            assert np.array_equal(a, b), k
