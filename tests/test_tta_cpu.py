"""Test-time augmentation (TEST.AUG), host side: the view plan, the float32 box rule of the views against the fixture recorded from the
reference's own `inference` (tests/golden/gen_tta_golden.py), the fixture's decision margins, the config keys, the C-ABI declarations and
the refusals."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tta_ref  # noqa: E402

H, W = 96, 128
RECORDED = ("tta", "tta_ft", "tta_noflip")          # "tta_mask": the reference raises (below)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "tta_golden.npz"))


def _aug(name):
    from unit_amd.config import CN
    sizes, max_size, flip = tta_ref.CASE_AUG[name]
    return CN(ENABLED=True, MIN_SIZES=sizes, MAX_SIZE=max_size, FLIP=flip)


@pytest.mark.parametrize("name", tta_ref.CASES)
def test_view_plan_matches_the_reference(gold, name):
    from unit_amd.modeling.inference import tta_view_plan
    plan = tta_view_plan(H, W, _aug(name))
    assert [list(map(int, v)) for v in plan] == gold[f"{name}/views"].tolist()
    assert plan == tta_ref.view_plan(H, W, *tta_ref.CASE_AUG[name])


def test_view_sizes_are_the_ones_the_cases_were_chosen_for(gold):
    v = gold["tta/views"].tolist()
    assert v == [[64, 85, 0], [64, 85, 1], [96, 128, 0], [96, 128, 1], [120, 160, 0], [120, 160, 1]]          # odd width, unchanged, max-size clamp
    assert gold["tta_noflip/views"].tolist() == [[64, 85, 0], [120, 160, 0]]


@pytest.mark.parametrize("name", tta_ref.CASES)
def test_float32_box_rule_bit_for_bit_and_float64_not(gold, name):
    props = gold[f"{name}/proposals"]
    assert props.dtype == np.float32 and props.shape == (tta_ref.N_PROPOSALS, 4)
    assert (props[:, 0] == 0).sum() >= 2 and (props[:, 2] == W).sum() >= 2 and (props[:, 2] == props[:, 0]).sum() >= 1
    differ = 0
    for i, (nh, nw, fl) in enumerate(gold[f"{name}/views"].tolist()):
        want = gold[f"{name}/view_boxes{i}"]
        got = tta_ref.view_boxes(props, H, W, nh, nw, bool(fl))
        assert want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, i)
        got64 = tta_ref.view_boxes(props, H, W, nh, nw, bool(fl), dtype=np.float64).astype(np.float32)
        differ += int((got64.view(np.uint32) != want.view(np.uint32)).sum())
        if fl:          # both clips matter: a box touching the right edge flips onto x0 = 0, no coordinate is clipped to the maximum
            assert (want[:, 0] == 0).any() and (want >= 0).all()
    print(f"{name}: float64 arithmetic differs from the recorded float32 boxes in {differ} elements")
    if any((nh, nw) != (H, W) for nh, nw, _ in gold[f"{name}/views"].tolist()):          # (a scale of exactly 1 and W - x are exact in both)
        assert differ > 0


@pytest.mark.parametrize("name", RECORDED)
def test_fixture_margins(gold, name):
    thr, nms_thr, topk = gold[f"{name}/thresholds"].tolist()
    m = tta_ref.detection_margins(gold[f"{name}/probs_sum"], gold[f"{name}/delta_mean"], gold[f"{name}/proposals"], (H, W), (10.0, 10.0, 5.0, 5.0),
                                  thr, nms_thr, int(topk))
    print(name, m)
    assert m["score"] >= tta_ref.MARGIN and m["iou"] >= tta_ref.MARGIN and m["topk"] >= tta_ref.MARGIN
    assert len(gold[f"{name}/scores"]) > 3 and len(gold[f"{name}/scores"]) <= m["n"]
    assert int(gold[f"{name}/has_masks"]) == 0
    n_views = len(gold[f"{name}/views"])
    ps = gold[f"{name}/probs_sum"]
    assert np.allclose(ps.sum(1), n_views, rtol=1e-5)          # the sum is NOT renormalised
    assert gold[f"{name}/scores"].max() > 1.0 or n_views == 1 or name == "tta_noflip"


def test_reference_cannot_run_tta_on_mask_heads(gold):
    """the fixture records where the reference's own TTA stops on its mask ROI heads; this project refuses instead"""
    assert int(gold["tta_mask/reference_raises_at"]) == 770
    assert "tta_mask/scores" not in gold.files
    from unit_amd.modeling.inference import TTA_MASK_HEADS, UnsupportedConfig, tta_check
    with pytest.raises(UnsupportedConfig, match="mask head") as e:
        tta_check(_aug("tta_mask"), [_inp(3)], 20, candidate_limit=65536, mask_on=True)
    assert str(e.value) == TTA_MASK_HEADS and "roi_heads.py:770" in TTA_MASK_HEADS


def test_config_keys():
    from unit_amd import config
    for c in (config.get_cfg(), config.voc_rcnn_c4_split1(50), config.coco_rcnn_c4_split1_segm(50)):
        a = c.TEST.AUG
        assert a.ENABLED is False          # the reference's default is True; every shipped yaml sets False and so does this project
        assert tuple(a.MIN_SIZES) == (480, 576, 688, 864, 1200) and a.MAX_SIZE == 2000 and a.FLIP is True


def test_exports_declared():
    from unit_amd._lib import parse_header, parse_header_names
    protos, names = parse_header(), parse_header_names()
    for fn in ("unit_image_chw_to_u8", "unit_tta_boxes", "unit_tta_accumulate"):
        assert fn in protos and names[fn][-1] == "stream", fn
    assert names["unit_tta_boxes"] == ["props", "count", "P", "Pcap", "views", "V", "out", "stream"]
    assert "unit_nms_max_candidates" in protos and names["unit_nms_max_candidates"] == []


def _inp(n, with_proposals=True):
    from unit_amd.structures import Boxes, Instances
    x = {"image": torch.zeros(3, H, W), "height": H, "width": W}
    if with_proposals:
        x["proposals"] = Instances((H, W), proposal_boxes=Boxes(torch.zeros(n, 4)))
    return x


def test_refusals():
    from unit_amd.modeling.inference import (TTA_DETECTED_INSTANCES, TTA_NEEDS_PROPOSALS, TTA_NO_SIZES, UnsupportedConfig, tta_check)
    aug = _aug("tta")
    tta_check(aug, [_inp(70)], 20, candidate_limit=65536)          # the fixture's call passes
    with pytest.raises(UnsupportedConfig, match="needs precomputed proposals") as e:
        tta_check(aug, [_inp(70), _inp(0, with_proposals=False)], 20, candidate_limit=65536)
    assert str(e.value) == TTA_NEEDS_PROPOSALS and "rcnn.py:515" in TTA_NEEDS_PROPOSALS
    with pytest.raises(NotImplementedError, match="detected_instances") as e:
        tta_check(aug, [_inp(70)], 20, detected_instances=[object()], candidate_limit=65536)
    assert str(e.value) == TTA_DETECTED_INSTANCES
    empty = _aug("tta")
    empty.MIN_SIZES = ()
    with pytest.raises(UnsupportedConfig, match="empty TEST.AUG.MIN_SIZES") as e:
        tta_check(empty, [_inp(70)], 20, candidate_limit=65536)
    assert str(e.value) == TTA_NO_SIZES


def test_candidate_overflow_refused_with_the_kernels_limit():
    """the limit is the NMS kernel's, read out of the built library (which loads without a device)"""
    from unit_amd import ops
    from unit_amd.modeling.inference import UnsupportedConfig, tta_check
    limit = ops.max_detection_candidates()
    assert limit == 65536          # NMS_SCAN_THREADS * 64 (csrc/sort_nms.hip)
    aug = _aug("tta")
    tta_check(aug, [_inp(limit // 20)], 20)
    with pytest.raises(UnsupportedConfig, match=f"exceed the {limit} the NMS kernel takes") as e:
        tta_check(aug, [_inp(limit // 20 + 1)], 20)
    assert f"at most {limit // 20} proposals" in str(e.value)
    tta_check(aug, [_inp(limit // 80)], 80)
    with pytest.raises(UnsupportedConfig):
        tta_check(aug, [_inp(limit // 80 + 1)], 80)


def test_model_inference_refuses_before_running():
    """at the call, on a model that was never moved to a device: the refusals come before any launch"""
    from unit_amd import config
    from unit_amd.modeling import build_model
    from unit_amd.modeling.inference import UnsupportedConfig, inference_tta
    cfg = config.voc_rcnn_c4_split1(50)
    cfg.MODEL.DEVICE = "cpu"
    cfg.TEST.AUG.ENABLED = True
    model = build_model(cfg)
    with pytest.raises(UnsupportedConfig, match="needs precomputed proposals"):
        inference_tta(model, [_inp(0, with_proposals=False)])
    with pytest.raises(NotImplementedError, match="detected_instances"):
        inference_tta(model, [_inp(5)], detected_instances=[types.SimpleNamespace()])


def test_both_meta_architectures_share_the_tta_path():
    """WeaklySupervisedRCNNRPN.inference (meta_arch/rcnn.py:658-690 carries the same TTA branch) is the base class's: one driver in modeling/inference.py"""
    from unit_amd.modeling.rcnn import WeaklySupervisedRCNNNoMeta, WeaklySupervisedRCNNRPN
    assert WeaklySupervisedRCNNRPN.inference is WeaklySupervisedRCNNNoMeta.inference
